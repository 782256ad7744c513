// enc_dense1.inc -- k_enc_dense1p: Dense(200) before its bias and activation (the head adds both); part of encoder.hip.
// Split-K GEMM  part[s][row][208] = F3[row][k0 : k0 + KTOT/S] x Wd1[k0 : k0 + KTOT/S][208], S = D1_SPLIT_OF(KTOT) -- f16 x 2 like conv3.
#define D1_BM 64
#define D1_BK 32      // one v_mfma_f32_16x16x32_f16 k-step per stage
#define D1_SPLIT 8  // the most k slices any instance uses: sizes the partial-sum buffer
// k slices per row tile: 8 for the long-K instance (K = 16384: 16 row tiles x 8 = 128 workgroups per frame); 4 for K = 2048 --
// one frame still fills the chip (48 x 4 workgroups, 29 us either way), a batch of 8 frames writes and re-reads half the partial
// sums (10.3 -> 10.6 k frames/s; 2 slices: 10.7 k but 48 us for a single frame).  One value for every launch size: the head adds
// the slices in order, so the descriptors' low bits depend on it and single calls must equal batched ones bit for bit.
#ifndef D1_SPLIT_2048
#define D1_SPLIT_2048 2   // k slices of Dense(200) (K = 2048).  Round 6: 4 -> 2 (half the partial sums written and read back by the head: head 22 -> 15 us, Dense(200) 83 -> 90 us per 24 576 rows, +1.5-3 % frames/s in 11 of 11 A/B runs, profiles/r06_dense1_split.txt; `make EXTRA=-DD1_SPLIT_2048=4 ...` builds the old one)
#endif
#define D1_SPLIT_OF(KTOT) ((KTOT) > 2048 ? 8 : D1_SPLIT_2048)
#define D1_THREADS 512
#define D1_NT (DENSE_NP / 16)          // 13 n-tiles
// Round 3: like conv3, Dense(200) evaluates its f32 products from TWO f16 terms per operand and three partial products
// (hi hi + hi lo + lo hi; the dropped lo lo term is 2^-22 relative): 3 MFMAs per K = 32 slab instead of the 6 of the 3-way bf16
// split, a 26 KB instead of a 39 KB weight stage (the LDS-DMA weight stream was this kernel's ceiling), two A planes instead of three.
#define D1_NS 2                        // terms per operand
#define D1_B16 (D1_NS * D1_NT * 64)    // uint4 of a B stage: [term][n-tile][lane]
#define D1_BSLOTS ((D1_B16 + D1_THREADS - 1) / D1_THREADS)

// host: Wd1 [K][200] -> per 32-deep k-step the LDS image of the B operand: [kstep][f16 term 2][n-tile 13][lane 64] x 16 B,
// lane (n = lane & 15, g = lane >> 4) holding k = 32 kstep + 8 g .. + 7 of column 16 ntile + n (zero beyond 200)
static void dense1_split_weights(const float *wd1, int K, uint4 *out) {
    for (int ks = 0; ks < K / 32; ++ks)
        for (int nt = 0; nt < D1_NT; ++nt)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = lane & 15, g = lane >> 4, col = nt * 16 + n;
                uint16_t h[8], l[8];
                for (int i = 0; i < 8; ++i)
                    enc_split2h(col < DENSE_N ? wd1[(size_t)(ks * 32 + 8 * g + i) * DENSE_N + col] : 0.0f, h[i], l[i]);
                uint4 *o = out + (size_t)ks * D1_B16 + nt * 64 + lane;
                o[0] = enc_pack_h8(h);
                o[D1_NT * 64] = enc_pack_h8(l);
            }
}

int enc_upload_dense1(const float *wd1, const float *bd1, int K, void **wx_dev, float **bd_dev) {
    const size_t n = (size_t)(K / 32) * D1_B16;
    uint4 *wx = (uint4 *)malloc(n * sizeof(uint4));
    if (!wx) { caelo_set_error("out of host memory"); return CAELO_ERR_ARG; }
    dense1_split_weights(wd1, K, wx);
    float bd[DENSE_NP] = {0.0f};
    memcpy(bd, bd1, DENSE_N * sizeof(float));
    hipError_t e = hipSuccess;
    if (!*wx_dev) e = hipMalloc(wx_dev, (n + 6 * 64) * sizeof(uint4));  // + six 1 KB pieces: k_enc_dense1p's waves copy 32 pieces per 26-piece stage
    if (e == hipSuccess && !*bd_dev) e = hipMalloc((void **)bd_dev, sizeof(bd));
    if (e == hipSuccess) e = hipMemcpy(*wx_dev, wx, n * sizeof(uint4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*bd_dev, bd, sizeof(bd), hipMemcpyHostToDevice);
    free(wx);
    if (e != hipSuccess) { caelo_set_error("dense_1 upload failed: %s", hipGetErrorString(e)); return CAELO_ERR_HIP; }
    return CAELO_OK;
}

typedef _Float16 d1_h8 __attribute__((ext_vector_type(8)));
#define D1_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_f16((A), (B), (C), 0, 0, 0)

// ------------------------------------------------------------------------------------------------
// dense1, software-pipelined.  Its two-barrier predecessor (k_enc_dense1, gone from the library) needed 90 KB of LDS, so ONE workgroup
// ran per CU, and its stage was a chain -- write A, barrier, fetch fragments from LDS, 42 MFMAs per wave, barrier -- in which the
// matrix pipe idled through every LDS round trip (SQ counters, 8-frame launch: MFMA busy 35 %, waves parked at waitcnt / barrier
// 51 % of their cycles).  This kernel keeps the one workgroup per CU and gives it the whole LDS: A double-buffered, THREE weight stages, so that
//   - the fragments of the next group of column tiles (and of the next stage, across the barrier) are in flight while the
//     current group's MFMAs run: the pipe has work on both sides of the single barrier of a stage;
//   - the weight DMA runs two stages ahead and the rows of F3 (HBM) two stages ahead in alternating registers; the barrier
//     waits with vmcnt(one stage's loads): only the older stage must have landed.
// The weight DMA, the F3 loads and the A stores are inline asm with hand-counted waits: with a compiler-visible LDS-DMA in the
// loop hipcc waits vmcnt(0) before every use of a loaded register and before every LDS store, and lgkmcnt(0) before every use
// of an LDS fragment (measured on a three-line kernel); without one its lgkmcnt arithmetic is exact.  Same products in the same order per accumulator in all three instances: bit-identical partial sums.
#define D1P_BSTRIDE (26 * 64)  // uint4 per weight buffer: the 26 pieces of 1 KB of a stage (waves 6 and 7 copy pieces 22..25, twice over: every wave issues
                               // four loads per stage, which the vmcnt arithmetic relies on, and nothing lands outside the buffer -- round 3's buffers
                               // were 32 KB for the six pieces the last waves brought along: 128 KB of LDS for the 128-row instance, now 110)
#define D1P_NBUF(MTW) 3
#define D1P_LDS_BYTES(MTW) ((2 * D1_NS * 4 * D1_BM * (MTW) + D1P_NBUF(MTW) * D1P_BSTRIDE) * 16)
// MTW = 1: 64 rows per workgroup, 94 KB.  MTW = 2: 128 rows, 110 KB -- every wave owns two row tiles, each weight fragment feeds
// two MFMAs, and the weight stream from L2 halves.  History of the 8-frame launch (24 576 rows): bf16 x 3 with 39 KB stages
// streamed 983 MB at 64 rows (125 us = 7.9 TB/s, the LDS-DMA ceiling of the chip) and 118 us at 128 rows with TWO weight buffers
// (all the LDS there was); f16 x 2 (26 KB stages, half the MFMAs) 101 us with two buffers -- a stage then cannot be shorter than
// one L2 -> LDS round trip, ~2 us under this load, whatever the matrix pipe does -- and 81 us with the third buffer the smaller
// stages leave room for (319 MB of weights + 201 MB of rows per launch = 6.4 TB/s).
template <int KTOT, int MTW>
__global__ void __launch_bounds__(D1_THREADS, 2) k_enc_dense1p(const float *__restrict__ f3, int64_t n_rows_pad,
                                                               const uint4 *__restrict__ wd1x, float *__restrict__ part,
                                                               const caelo_enc_in in) {
    constexpr int BM = D1_BM * MTW, A16 = D1_NS * 4 * BM, NBUF = D1P_NBUF(MTW), NKS = KTOT / D1_SPLIT_OF(KTOT) / D1_BK;
    constexpr int DMA = 4;              // 1 KB pieces a wave copies per stage (8 waves x 4 = 32 >= 26)
    constexpr int PER_STAGE = DMA + MTW;  // loads a thread has in flight per stage: its DMA pieces + its rows
    static_assert(MTW >= 1 && MTW <= 3, "three instances");
    static_assert(NKS % 2 == 0 && NKS >= 6, "stages are unrolled in pairs, the last ones peeled");
    // workgroup -> (row tile, k slice).  De-duplicated launch: only the tiles that hold distinct patches of their frame do work
    // (tiles never straddle frames), and they are numbered FIRST: with one workgroup per CU (LDS) an idle workgroup in the
    // middle of the dispatch order still waits for a whole CU to drain before it can start and exit (96 us for the 62 %
    // of a launch's tiles that are live, against 111 us for all of them, when the idle ones sat where their rows are).
    int64_t row0 = (int64_t)blockIdx.x * BM;
    int split = blockIdx.y;
    if (in.dedup) {
        const int lin = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        int t = lin / D1_SPLIT_OF(KTOT), f = 0;
        split = lin - t * D1_SPLIT_OF(KTOT);
        for (; f < in.n_frames; ++f) {
            const int live = (enc_tables(in, f)->count + BM - 1) / BM;
            if (t < live) break;
            t -= live;
        }
        if (f == in.n_frames) return;
        row0 = (int64_t)f * in.per_frame + (int64_t)t * BM;
    }
    extern __shared__ uint4 d1_lds[];
    uint4 *As = d1_lds;            // [2][split][g][row]
    uint4 *Bs = d1_lds + 2 * A16;  // [NBUF][split][n-tile][lane] (+ 1 KB)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, n = lane & 15;
    const int ks0 = split * NKS;
    const int mg = wave >> 1;          // rows mg * 16 MTW ... of the tile
    const bool odd = (wave & 1) != 0;  // n-tiles 7..12 (6 of them) instead of 0..6
    const int nt0 = odd ? 7 : 0;
    f32x4 acc[MTW][7];
#pragma unroll
    for (int q = 0; q < MTW; ++q)
#pragma unroll
        for (int i = 0; i < 7; ++i) acc[q][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // A fetch: rows a_row (+ 64), 4 consecutive k (16 bytes) from 4 a_kq.  Lane -> (row, a_kq) so that the 16 lanes one LDS store
    // cycle serves (8 rows x the two halves of a 16-byte unit) fall into 16 different bank pairs; (tid >> 3, tid & 7) put four
    // lanes on every bank: 288 conflict cycles per stage, 20 us of the 8-frame launch.  A wave still reads 8 rows x 128 bytes.
    const int a_row = wave * 8 + ((lane >> 1) & 7), a_kq = ((lane >> 4) << 1) | (lane & 1);
    const float *a_src = f3 + (size_t)(row0 + a_row) * KTOT + (size_t)ks0 * D1_BK + a_kq * 4;
    // this wave's second piece (pb + 1) of weight buffer 0 in LDS (the DMA adds 16 x lane itself) and of stage ks0 in memory
    const int pb = wave < 6 ? 4 * wave : 22;   // first of this wave's four pieces
    const uint32_t b_lds = (uint32_t)(uintptr_t)(void __attribute__((address_space(3))) *)(Bs + (pb + 1) * 64);
    const uint4 *b_mid = wd1x + (size_t)ks0 * D1_B16 + (pb + 1) * 64 + lane;
    // LDS byte address of this thread's 8 bytes of A buffer 0, high term ([split][g = a_kq >> 1][row] x 16 B, half a_kq & 1)
    const uint32_t a_lds = (uint32_t)(uintptr_t)(void __attribute__((address_space(3))) *)&As[(a_kq >> 1) * BM + a_row] + (a_kq & 1) * 8;
    f32x4 paA[MTW], paB[MTW];
    d1_h8 af0[MTW][D1_NS], af1[MTW][D1_NS], bf0[4][D1_NS], bf1[3][D1_NS];
    // four CONSECUTIVE 1 KB pieces per wave and stage, addressed from the second one by the instruction's immediate offset (it
    // moves the global and the LDS address alike): one M0 write and one address register per stage instead of four of each.
    // Waves 6 and 7 both copy pieces 22..25 (D1P_BSTRIDE above): every wave has the same count of loads in flight, which the
    // vmcnt arithmetic below relies on.
#define D1P_FETCH_B(KS, BUF)                                                                                     \
    {                                                                                                            \
        const uint4 *gp_ = b_mid + (size_t)(KS) * D1_B16;                                                        \
        const uint32_t la_ = b_lds + (uint32_t)(BUF) * (D1P_BSTRIDE * 16u);                                      \
        __asm__ volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\t"                                                       \
                         "global_load_lds_dwordx4 %1, off offset:-1024\n\t"                                       \
                         "global_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %1, off offset:1024\n\t"    \
                         "global_load_lds_dwordx4 %1, off offset:2048" : : "s"(la_), "v"(gp_) : "memory");       \
    }
#define D1P_LOAD_A(P, KS)                                                                                        \
    _Pragma("unroll") for (int r = 0; r < MTW; ++r) {                                                            \
        const float *p_ = a_src + (size_t)(64 * r) * KTOT + (size_t)(KS) * D1_BK;                                \
        __asm__ volatile("global_load_dwordx4 %0, %1, off" : "=v"(P[r]) : "v"(p_) : "memory");                   \
    }
    // wait until at most N loads are in flight; the registers are operands so that no use moves above the wait
#define D1P_WAIT_A(P, N)                                                                                         \
    {                                                                                                            \
        if (MTW == 1) __asm__ volatile("s_waitcnt vmcnt(%1)" : "+v"(P[0]) : "n"(N) : "memory");                  \
        else __asm__ volatile("s_waitcnt vmcnt(%2)" : "+v"(P[0]), "+v"(P[MTW - 1]) : "n"(N) : "memory");         \
    }
    // (the stores are inline asm as well: a compiler-visible LDS store is ordered behind every LDS-DMA in flight -- vmcnt(0))
#define D1P_STORE_A(P, ABUF)                                                                               \
    _Pragma("unroll") for (int r = 0; r < MTW; ++r) {                                                      \
        uint32_t h01_, l01_, h23_, l23_;                                                                   \
        enc_split2h_pk(P[r][0], P[r][1], h01_, l01_);                                                      \
        enc_split2h_pk(P[r][2], P[r][3], h23_, l23_);                                                      \
        const unsigned long long dh_ = ((unsigned long long)h23_ << 32) | h01_, dl_ = ((unsigned long long)l23_ << 32) | l01_; \
        if (r == 0)                                                                                        \
            __asm__ volatile("ds_write_b64 %0, %1 offset:%3\n\tds_write_b64 %0, %2 offset:%4"               \
                             : : "v"(a_lds), "v"(dh_), "v"(dl_), "n"((ABUF) * A16 * 16),                     \
                                 "n"((ABUF) * A16 * 16 + 4 * BM * 16) : "memory");                          \
        else if (r == 1)                                                                                   \
            __asm__ volatile("ds_write_b64 %0, %1 offset:%3\n\tds_write_b64 %0, %2 offset:%4"               \
                             : : "v"(a_lds), "v"(dh_), "v"(dl_), "n"((ABUF) * A16 * 16 + 1024),              \
                                 "n"((ABUF) * A16 * 16 + 4 * BM * 16 + 1024) : "memory");                   \
        else                                                                                               \
            __asm__ volatile("ds_write_b64 %0, %1 offset:%3\n\tds_write_b64 %0, %2 offset:%4"               \
                             : : "v"(a_lds), "v"(dh_), "v"(dl_), "n"((ABUF) * A16 * 16 + 2048),              \
                                 "n"((ABUF) * A16 * 16 + 4 * BM * 16 + 2048) : "memory");                   \
    }
#define D1P_READ_A(AF, ABUF)                                                                               \
    _Pragma("unroll") for (int q = 0; q < MTW; ++q) {                                                      \
        const uint4 *ap_ = &As[(ABUF) * A16 + g * BM + (mg * MTW + q) * 16 + n];                           \
        AF[q][0] = __builtin_bit_cast(d1_h8, ap_[0]);                                                      \
        AF[q][1] = __builtin_bit_cast(d1_h8, ap_[4 * BM]);                                                 \
    }
    // column tiles nt0 .. nt0+3 (group 0) and nt0+4 .. nt0+6 (group 1).  Odd waves own six tiles: their seventh accumulator
    // repeats tile 12 and is dropped at the end -- no branches in the stage; the SIMDs that run the odd waves have the idle
    // slots (36 instead of 42 MFMAs per row tile and stage)
#define D1P_READ_B0(BUF)                                                                                   \
    {                                                                                                      \
        const uint4 *bp_ = &Bs[(BUF) * D1P_BSTRIDE + nt0 * 64 + lane];                                     \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                      \
        _Pragma("unroll") for (int sp = 0; sp < D1_NS; ++sp) bf0[i][sp] = __builtin_bit_cast(d1_h8, bp_[(sp * D1_NT + i) * 64]); \
    }
#define D1P_READ_B1(BUF)                                                                                   \
    {                                                                                                      \
        const uint4 *bp_ = &Bs[(BUF) * D1P_BSTRIDE + lane];                                                \
        _Pragma("unroll") for (int i = 0; i < 3; ++i) {                                                    \
            const int t_ = (i == 2 && odd) ? D1_NT - 1 : nt0 + 4 + i;                                      \
            _Pragma("unroll") for (int sp = 0; sp < D1_NS; ++sp) bf1[i][sp] = __builtin_bit_cast(d1_h8, bp_[(sp * D1_NT + t_) * 64]); \
        }                                                                                                  \
    }
    // smallest terms first (AF / B index: 0 high, 1 low); the accumulators alternate
#define D1P_TERM0(AF, SA, SB)                                                                              \
    _Pragma("unroll") for (int q = 0; q < MTW; ++q)                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                          \
        acc[q][i] = D1_MFMA(AF[q][SA], bf0[i][SB], acc[q][i]);
#define D1P_MFMA_G0(AF) D1P_TERM0(AF, 1, 0) D1P_TERM0(AF, 0, 1) D1P_TERM0(AF, 0, 0)
#define D1P_TERM1(AF, SA, SB)                                                                              \
    _Pragma("unroll") for (int q = 0; q < MTW; ++q)                                                        \
    _Pragma("unroll") for (int i = 0; i < 3; ++i)                                                          \
        acc[q][4 + i] = D1_MFMA(AF[q][SA], bf1[i][SB], acc[q][4 + i]);
#define D1P_MFMA_G1(AF) D1P_TERM1(AF, 1, 0) D1P_TERM1(AF, 0, 1) D1P_TERM1(AF, 0, 0)
    // One stage ST whose successor exists.  On entry: bf0 / AFC hold (or are receiving) stage ST's first group and A fragments;
    // in flight, oldest first: weight DMA ST+1 (5), rows ST+1 (registers PN), then YOUNGER more loads of later stages.
    // ISSUE: start DMA ST+NBUF (into the buffer stage ST leaves) and its rows (into PN).  BC / BN: weight buffers of ST / ST+1.
#define D1P_STAGE(ST, AFC, AFN, PN, ABN, BC, BN, YOUNGER, ISSUE)                                                    \
    {                                                                                                               \
        D1P_READ_B1(BC)                                                                                             \
        __builtin_amdgcn_sched_barrier(0); /* the reads stay ahead of the MFMAs that cover them */                  \
        D1P_MFMA_G0(AFC)                                                                                            \
        D1P_WAIT_A(PN, YOUNGER)                                                                                     \
        D1P_STORE_A(PN, ABN)                                                                                        \
        /* rows ST+1 are written, weights ST+1 have landed (older than the rows just waited for), every wave is */  \
        /* done reading stage ST's buffers */                                                                       \
        __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
        if (ISSUE) {                                                                                                \
            D1P_FETCH_B((ST) + NBUF, BC)                                                                            \
            D1P_LOAD_A(PN, (ST) + NBUF)                                                                             \
        }                                                                                                           \
        D1P_READ_A(AFN, ABN)                                                                                        \
        D1P_READ_B0(BN)                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
        D1P_MFMA_G1(AFC)                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
    }
    D1P_FETCH_B(0, 0)
    D1P_LOAD_A(paA, 0)
    D1P_FETCH_B(1, 1)
    D1P_LOAD_A(paB, 1)
    D1P_FETCH_B(2, 2)
    D1P_WAIT_A(paA, PER_STAGE + DMA)  // stage 0: its weights (older) and its rows
    D1P_STORE_A(paA, 0)
    D1P_LOAD_A(paA, 2)
    __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    D1P_READ_A(af0, 0)
    D1P_READ_B0(0)
    int b0 = 0;  // weight buffer of stage st (st % 3)
#pragma unroll 1
    for (int st = 0; st < NKS - 4; st += 2) {
        const int b1 = b0 == 2 ? 0 : b0 + 1, b2 = b1 == 2 ? 0 : b1 + 1;
        D1P_STAGE(st, af0, af1, paB, 1, b0, b1, PER_STAGE, true)
        D1P_STAGE(st + 1, af1, af0, paA, 0, b1, b2, PER_STAGE, true)
        b0 = b2;
    }
    constexpr int c0 = (NKS - 4) % 3, c1 = (NKS - 3) % 3, c2 = (NKS - 2) % 3, c3 = (NKS - 1) % 3;
    D1P_STAGE(NKS - 4, af0, af1, paB, 1, c0, c1, PER_STAGE, true)
    D1P_STAGE(NKS - 3, af1, af0, paA, 0, c1, c2, PER_STAGE, false)
    D1P_STAGE(NKS - 2, af0, af1, paB, 1, c2, c3, 0, false)
    // the last stage: its first group and A fragments are on their way, nothing to prepare
    D1P_READ_B1(c3)
    __builtin_amdgcn_sched_barrier(0);
    D1P_MFMA_G0(af1)
    D1P_MFMA_G1(af1)
    // C rows 4g + r of each tile
#pragma unroll
    for (int q = 0; q < MTW; ++q)
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            if (i == 6 && odd) continue;
            float *dst = part + ((size_t)split * n_rows_pad + row0 + (mg * MTW + q) * 16 + 4 * g) * DENSE_NP + (nt0 + i) * 16 + n;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(size_t)r * DENSE_NP] = acc[q][i][r];
        }
}

// (per_device_once: caelo_internal.h)
template <int KTOT>
static int dense1_launch(int device, const float *f3, int64_t np, const void *wd1x, float *part, const caelo_enc_in &in, hipStream_t s) {
    // once per device (under a lock: the pipeline's encoder thread and the caller may race here)
    static hipError_t attr_slot[CAELO_MAX_DEVICES];
    static bool attr_have[CAELO_MAX_DEVICES];
    static std::mutex attr_mu;
    const hipError_t attr = per_device_once(device, attr_slot, attr_have, attr_mu, [] {
        hipError_t e = hipFuncSetAttribute((const void *)k_enc_dense1p<KTOT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, D1P_LDS_BYTES(1));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)k_enc_dense1p<KTOT, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, D1P_LDS_BYTES(2));
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)k_enc_dense1p<KTOT, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, D1P_LDS_BYTES(3));
        return e;
    });
    CAELO_HIP(attr);
    // CAELO_D1_WIDE_FROM: launch size (rows) from which the 128-row instance is used -- a tuning threshold, the partial sums of the two
    // instances are bit-identical (tests/test_gpu_parity.py::test_dense1_tile_sizes_are_bit_identical)
    static const int64_t wide_from = getenv("CAELO_D1_WIDE_FROM") ? atoll(getenv("CAELO_D1_WIDE_FROM")) : 4 * 3072;  // rows
    // 192-row tiles (round 6) for launches of EVERY patch (no de-duplication) that 128-row tiles would take two rounds over (more than
    // 256 x 64 rows): one and a half times the MFMAs per weight fragment, two thirds of the weight stream, one round -- 90 -> 68 us per
    // 24 576 rows; 12 288 rows (one round either way) 45 -> 56 us, which is why de-duplicated launches (~13 k live rows of a batch, a
    // number the host does not know) stay on 128-row tiles: 19.7 against 19.5 k frames/s (profiles/r06_dense1_tile192.txt).  Same partial sums.
    static const int64_t tile3_from = getenv("CAELO_D1_TILE3_FROM") ? atoll(getenv("CAELO_D1_TILE3_FROM")) : 256 * 64 + 1;  // rows
    if (KTOT == 2048 && !in.dedup && np % 192 == 0 && np >= tile3_from && np >= wide_from) {
        dim3 gw((unsigned)(np / 192), D1_SPLIT_OF(KTOT));
        k_enc_dense1p<KTOT, 3><<<gw, D1_THREADS, D1P_LDS_BYTES(3), s>>>(f3, np, (const uint4 *)wd1x, part, in);
    } else
    if (np % 128 == 0 && (!in.dedup || in.per_frame % 128 == 0) && (np >= wide_from || KTOT > 2048)) {  // (tiles never straddle frames)
        // 128-row tiles once the launch fills the chip with them, and always for the long-K instance (8 k slices per row tile):
        // half the weight stream; same partial sums
        dim3 gw((unsigned)(np / 128), D1_SPLIT_OF(KTOT));
        k_enc_dense1p<KTOT, 2><<<gw, D1_THREADS, D1P_LDS_BYTES(2), s>>>(f3, np, (const uint4 *)wd1x, part, in);
    } else {
        dim3 gd((unsigned)(np / 64), D1_SPLIT_OF(KTOT));
        k_enc_dense1p<KTOT, 1><<<gd, D1_THREADS, D1P_LDS_BYTES(1), s>>>(f3, np, (const uint4 *)wd1x, part, in);
    }
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}
