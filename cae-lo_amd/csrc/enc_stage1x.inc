// enc_stage1x.inc -- k_enc_stage1x, round 3's stage 1 (conv1 + pool1 + conv2 + pool2 of the 3D-CAE encoder); part of encoder.hip.
//
// Reference behaviour restated (never its code): the first four layers of EncoderModel4VoxelPatch.h5 as
// GetFeaturesFromPatches runs them (Match.py:130-135): Conv3D(1->8,3^3,same) tanh -> MaxPool3D(2) -> Conv3D(8->16) tanh ->
// MaxPool3D(2), on bit-packed 16^3 patches, P2 [patch][4][4][4][16] f32 out.
//
// Same structure as k_enc_stage1 (a patch per 4-wave workgroup, persistent grid, work counter, background-delta conv2 with
// exact skipping of all-background input rows) with the three things round 2's counters pointed at changed:
//   * conv1 left the VALU.  A pooled cell's eight conv1 positions all read the cell's 4x4x4 receptive field, 64 voxels =
//     the cell's 64-bit mask: out[cell][(sub-position, channel)] = mask[cell][64] . Wf[64][64], Wf = w1 scattered by
//     (voxel - sub-position).  One GEMM per 16 queued cells on v_mfma_f32_16x16x32_f16: the A operand is the mask expanded to
//     0.0 / 1.0 halves (exact), B = Wf as two f16 terms from LDS, pooling = max over the 4 n-tiles and one DPP rotate.
//   * every f32 product of conv1 / conv2 is evaluated on the f16 matrix pipe from 2-way splits x = hi + lo, hi = f16(x),
//     lo = f16(x - hi): |x - hi - lo| <= max(2^-22 |x|, 2^-25) (the MFMA honours f16 subnormals -- tools/micro/f16_mfma_subnormal.hip, measured
//     on MI355X -- so the low part of a small value is not lost).  All four partial products are summed:
//     K = 32 of one MFMA = 3 z-taps x 8 channels of one term + 8 slots for a 4th (tap, term), so a tap row of a tile costs
//     THREE 16-cycle MFMAs where k_enc_stage1 issued six 32-cycle f32 ones.  Against the f64-exact network the descriptors
//     move by 2e-7 (tools/emulate_split_precision.py; the f32 oracle itself is 1.3e-6 away from it).
//   * a tile pair walks its 12 input slabs (x plane, y row pair) once and feeds both tiles from each A fragment.  The
//     fragments of an ACTIVE input plane are fetched together and unconditionally (straight-line loads, so that hipcc counts
//     the waits itself: lgkmcnt(N)); only the MFMAs sit behind the per-slab activity tests, and a plane without an active slab
//     is skipped with its loads (round 4; round 3 fetched all 36 fragments of an active pair through a three-slab register ring).
//     (A hand-counted inline-asm pipeline with conditional loads was built first and measured 25 % SLOWER: hipcc tied the
//     waits to copies of the accumulators and serialised the MFMAs.)
//   * every phase is one LDS round trip deep where round 2 paid three to five: the next item's index and voxel rows are
//     fetched a patch ahead (work items from eight per-XCD queues), list lengths travel in registers, the wipe of the
//     previous patch's cells rides in the mask phase (three barriers per patch), and nothing in the loop waits on vmcnt
//     behind the P2 stores.  Two workgroups per CU with 256 registers.
// D in LDS (round 4): position q = (x*10 + yp)*10 + zp, x = 0..7 (NO x halo: a tap row whose input plane lies outside the patch
// is all background -- its MFMAs are skipped like any other all-background row and its fragment loads are pointed at plane 0 / 7),
// yp, zp = 0..9 with a zero halo (the two out-of-range y rows / z taps of a tile read stored zeros).  A position holds 32 B = two
// 16-byte units: [d_hi of channels 0..7] and [d_lo of channels 0..7], in that order in even padded-y rows and SWAPPED in odd ones
// (with the A rows ordered (yl, z / 4) = (0,0), (1,0), (1,1), (0,1) every ds_read_b128 of the three fragments below then touches each
// LDS bank once -- /tmp-style brute force over pitches and swizzles, tools/lds_layout_search.py).  The K = 32 of an MFMA is four
// 8-slot groups, group g = (z tap, term) of all 8 channels:
//     fragment 0: d_hi at taps (0, 1, 2, 0)      x  B_X = (w_hi t0, w_hi t1, w_hi t2, w_lo t0)
//     fragment 1: d_lo at taps (0, 1, 2, 0)      x  B_X  (the SAME registers)
//     fragment 2: (d_hi t1, d_hi t2, d_lo t1, d_lo t2)  x  B_Y = (w_lo t1, w_lo t2, w_lo t1, w_lo t2)
// -- all twelve (tap, term x term) products of a tap row in three MFMAs as before, but the B operand of a tap row is 8 registers
// instead of 12 (round 3 paired [d_hi x 4 | d_lo x 4] with a weight quadruple stored twice): 72 instead of 108 for the nine tap
// rows.  With the C0 accumulator start read from a 27-class table in LDS instead of 32 registers the kernel fits 168 registers and
// 53 KB of LDS: THREE workgroups per CU (round 3: two, 253 registers, 58 KB).
typedef _Float16 enc_h8 __attribute__((ext_vector_type(8)));
#define S1X_DQ 808     // 8 x 10 x 10 positions + 8 (fragment loads of the last plane run two z taps past the end)
#define S1X_RP 20
#define S1X_W1F_U4 (16 * 64)   // conv1 B operand: [k-step 2][n-tile 4][term 2][lane 64] uint4
#define S1X_W2X_U4 (18 * 64)   // conv2 B operand: [tap row 9][X, Y][lane 64] uint4
#define S1X_BGO_OFF (512 * 16 + 16)   // floats of the C0 table in front of k_enc_bgo_table's [16 pairs][64 lanes] float2

// conv2 A fragment f, k group g -> z tap and term (0 = d_hi, 1 = d_lo); B fragment b (0 = X, 1 = Y), group g -> z tap and weight term
__host__ __device__ constexpr int s1x_tap(int f, int g) { return f < 2 ? (g == 3 ? 0 : g) : 1 + (g & 1); }
__host__ __device__ constexpr int s1x_term(int f, int g) { return f == 0 ? 0 : (f == 1 ? 1 : (g >> 1)); }
__host__ __device__ constexpr int s1x_btap(int b, int g) { return b == 0 ? (g == 3 ? 0 : g) : 1 + (g & 1); }
__host__ __device__ constexpr int s1x_bterm(int b, int g) { return b == 0 ? (g == 3 ? 1 : 0) : 1; }
// A / C row group gq = m >> 2 -> (yl, z >> 2)
__host__ __device__ constexpr int s1x_yl(int gq) { return gq == 1 || gq == 2; }
__host__ __device__ constexpr int s1x_zh(int gq) { return gq >> 1; }

// host: the two B operands.  w1 [27][8], w2 [27][8][16] (Keras order).
static void stage1x_split_weights(const float *w1, const float *w2, uint4 *w1f, uint4 *w2x) {
    for (int ks = 0; ks < 2; ++ks)
        for (int nt = 0; nt < 4; ++nt)
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, n = lane & 15;
                const int col = nt * 16 + n, s = col >> 3, ch = col & 7;
                const int sa = s >> 2, sb = (s >> 1) & 1, sc = s & 1;
                uint16_t h[8], l[8];
                for (int i = 0; i < 8; ++i) {
                    const int k = ks * 32 + 8 * g + i;  // field voxel (a, b, j) = mask bit a*16 + b*4 + j
                    const int ka = (k >> 4) - sa, kb = ((k >> 2) & 3) - sb, kc = (k & 3) - sc;
                    const bool in = ka >= 0 && ka < 3 && kb >= 0 && kb < 3 && kc >= 0 && kc < 3;
                    enc_split2h(in ? w1[((ka * 3 + kb) * 3 + kc) * 8 + ch] : 0.0f, h[i], l[i]);
                }
                uint4 *o = w1f + (size_t)((ks * 4 + nt) * 2) * 64 + lane;
                o[0] = enc_pack_h8(h);
                o[64] = enc_pack_h8(l);
            }
    // conv2: B fragment b of tap row (ka, kb), lane (g, n): group g carries the 8 input channels of (z tap, weight term) = s1x_btap /
    // s1x_bterm [b][g] for output channel n
    for (int row = 0; row < 9; ++row)
        for (int b = 0; b < 2; ++b)
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, n = lane & 15;
                const int tap = row * 3 + s1x_btap(b, g);
                uint16_t v[8];
                for (int i = 0; i < 8; ++i) {
                    uint16_t h, l;
                    enc_split2h(w2[(tap * 8 + i) * 16 + n], h, l);
                    v[i] = s1x_bterm(b, g) ? l : h;
                }
                w2x[(size_t)(row * 2 + b) * 64 + lane] = enc_pack_h8(v);
            }
}

struct Stage1xLds {
    uint4 wf[16][64];                  // conv1 B operand.  FIRST in the struct: conv2's fragment loads of the (never active) input plane -1
                                       // of the first tile pair reach 3.2 KB below d, those of plane 8 3.2 KB above it (into c0cls / lmask)
    uint4 d[2 * S1X_DQ];               // D = P1 - BG: two 16-byte units per position, d_hi / d_lo of the 8 channels (swapped in odd y rows)
    float c0cls[27][16];               // conv2's accumulator start C0 = b2 + conv2(background) by border class (x, y, z in {0, inner, 7})
    unsigned long long lmask[512];     // receptive-field masks of the queued cells, by list slot
    unsigned short lcell[2][512];      // the queued cells (current patch / the one whose D entries are still to be wiped)
    unsigned int rows[2][18 * S1X_RP]; // voxel rows of a patch as (row << 1) words with a zero border: [x + 1][y + 1]
    unsigned int nzrow[12];            // per padded x plane: bit yp set when some cell (xp, yp, *) is non-background
    unsigned int planes[2][4];         // per rows buffer and wave: its four x rows' "holds a voxel" bits
    int list_n[2];
    int next_j[2];                     // [k & 1]: the item after the one being processed in iteration k
#ifdef CAELO_ENC_PROF
    unsigned int prof[16];
#endif
};

#ifdef CAELO_ENC_PROF  // make PROF=1: slots 0..5 = shader-clock cycles wave 0 spends in: wipe + masks + queue, barrier, conv1, barrier, end of patch, barrier; 6 = patches; 7 = queued cells; 8 = conv2's pairs, 9 = taking up the next rows / item, 10 = P2 stores (the compiler moves arithmetic across the clock reads: boundaries inside a barrier interval are approximate)
#define S1X_STAMP(i) do { if (threadIdx.x == 0) { const unsigned t_ = (unsigned)clock64(); L.prof[i] += t_ - s1x_t_prev; s1x_t_prev = t_; } } while (0)
#else
#define S1X_STAMP(i) do { } while (0)
#endif

#define S1X_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(enc_h8, (A)), __builtin_bit_cast(enc_h8, (B)), (C), 0, 0, 0)

// item J of the launch -> output row, source words.  Plain launches: coarsest scale first.  De-duplicated launches: frame by frame
// through the per-frame lists; the frame counts were read once (cum[]), so the only memory access here is the list entry.
struct S1xItems {
    int cumv;      // lane f < frames: items of the frames 0 .. f (INT_MAX in the other lanes): the frame of item J is the number of lanes with cumv <= J
    int n_items, nk, group;
};
__device__ inline void s1x_item(const caelo_enc_in &in, const S1xItems &it, int J, const unsigned long long *&src, int &row) {
    if (in.dedup) {
        // (round 3 walked a select chain over the eight frame counts held in scalar registers: ~70 instructions per item and wavefront,
        // part of what an item costs when there is little to compute.  A ballot over per-lane cumulative counts: five.)
        const int f = __popcll(__ballot(J >= it.cumv));
        const int first = f ? __builtin_amdgcn_readlane(it.cumv, f - 1) : 0;
        const int i = J - first;
        row = f * in.per_frame + i;
        src = in.bits + (size_t)f * in.frame_stride + (size_t)enc_tables(in, f)->list[i] * 64;
    } else {
        int sc = 0, kp = J;   // J = sc * nk + kp, sc < group: compare-subtract (group is 1 or 3; a division costs ~40 instructions)
        for (int t = 1; t < it.group; ++t)
            if (kp >= it.nk) { kp -= it.nk; ++sc; }
        row = kp * it.group + (it.group - 1 - sc);
        src = in.bits + (size_t)row * 64;
    }
}

// pooled outputs (pool2 + tanh) of a tile pair whose input rows are all background, for pair (xp, yi) = blockIdx.x and every lane of
// the wavefront that owns it: what the kernel's epilogue would compute from the C0 accumulator starts alone.  Written once per
// model behind the C0 table; an all-background pair is then one 8-byte load per lane that nothing waits for until the patch is stored.
template <int H>
static __device__ __forceinline__ void enc_bgo_table_body(float *c0g) {
    const int lane = threadIdx.x, g = lane >> 4, n = lane & 15;
    const int xp = blockIdx.x >> 2, yi = blockIdx.x & 3;
    f32x4 c[2];
#pragma unroll
    for (int xt = 0; xt < 2; ++xt) {
        const float *c0a = c0g + (size_t)((((2 * xp + xt) * 8 + 2 * yi + s1x_yl(g)) * 8 + 4 * s1x_zh(g)) * 16 + n);
        c[xt] = (f32x4){c0a[0], c0a[16], c0a[32], c0a[48]};
    }
    float v0 = fmaxf(fmaxf(c[0][0], c[0][1]), fmaxf(c[1][0], c[1][1]));
    float v1 = fmaxf(fmaxf(c[0][2], c[0][3]), fmaxf(c[1][2], c[1][3]));
    v0 = fmaxf(v0, __shfl_xor(v0, 16));   // the y pair sits in lane groups g and g ^ 1
    v1 = fmaxf(v1, __shfl_xor(v1, 16));
    ((float2 *)(c0g + S1X_BGO_OFF))[blockIdx.x * 64 + lane] = make_float2(enc_act<H>(v0), enc_act<H>(v1));
}
__global__ void __launch_bounds__(64) k_enc_bgo_table(float *c0g) { enc_bgo_table_body<CAELO_ACT_TANH>(c0g); }
__global__ void __launch_bounds__(64) k_enc_bgo_table_relu(float *c0g) { enc_bgo_table_body<CAELO_ACT_RELU>(c0g); }

// (the body of k_enc_stage1x and of its relu sibling: H = the hidden activation of conv1 and conv2)
template <int H, bool COUNT>
static __device__ __forceinline__ void enc_stage1x_body(const caelo_enc_in &in, int64_t n_patches, int group, int *__restrict__ work_counter,
                                                        const uint4 *__restrict__ w1f, const float *__restrict__ b1g,
                                                        const uint4 *__restrict__ w2x, const float *__restrict__ c0g,
                                                        float *__restrict__ p2out, unsigned long long *__restrict__ mfma_count) {
    __shared__ __attribute__((aligned(16))) Stage1xLds L;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int n = lane & 15;
    unsigned int n_mfma = 0;
    // ---- one-time: conv2's B operand (18 fragments = 72 registers); the C0 accumulator starts by border class go to LDS
    uint4 bq[9][2];
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) bq[r][j] = w2x[(r * 2 + j) * 64 + lane];
    for (int i = tid; i < 27 * 16; i += 256) {
        const int cls = i >> 4, ch = i & 15;
        const int cx = cls / 9, cy = (cls / 3) % 3, cz = cls % 3;   // class 0 / 1 / 2 = coordinate 0 / inner (3) / 7
        (&L.c0cls[0][0])[i] = c0g[(size_t)((((cx == 0 ? 0 : (cx == 1 ? 3 : 7)) * 8 + (cy == 0 ? 0 : (cy == 1 ? 3 : 7))) * 8 + (cz == 0 ? 0 : (cz == 1 ? 3 : 7))) * 16 + ch)];
    }
    for (int i = tid; i < S1X_W1F_U4; i += 256) (&L.wf[0][0])[i] = w1f[i];
    for (int i = tid; i < 2 * S1X_DQ; i += 256) L.d[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = tid; i < 2 * 18 * S1X_RP; i += 256) (&L.rows[0][0])[i] = 0u;
    if (tid < 12) L.nzrow[tid] = 0u;
    if (tid < 2) L.list_n[tid] = 0;
    const float b1c = b1g[n & 7], bgc = c0g[512 * 16 + (n & 7)];  // this lane's conv1 channel: bias and background tanh(b1)
    // the pooled outputs of this wavefront's four tile pairs when nothing but background feeds them: (xp, yi) is fixed per wavefront,
    // so the eight values are loaded ONCE instead of per item
    float2 bgo[4];
#pragma unroll
    for (int yi = 0; yi < 4; ++yi) bgo[yi] = ((const float2 *)(c0g + S1X_BGO_OFF))[((wave ^ S1_XDEAL(yi)) * 4 + yi) * 64 + lane];
    S1xItems it;
    it.nk = (int)(n_patches / group);
    it.group = group;
    {
        int cum = 0, mine = 0x7FFFFFFF;
#pragma unroll
        for (int f = 0; f < CAELO_ENC_MAX_FRAMES; ++f) {
            cum += (in.dedup && f < in.n_frames) ? __builtin_amdgcn_readfirstlane(enc_tables(in, f)->count) : 0;
            if (in.dedup && f < in.n_frames && lane == f) mine = cum;
        }
        it.cumv = mine;
        it.n_items = in.dedup ? cum : (int)n_patches;
    }
    const int n_items = it.n_items;
    if (blockIdx.x == 0 && tid < 8) work_counter[C3X_TICKET_INT + 32 * tid] = 0;   // conv3 (the next kernel on this stream) draws its pairs from here
    // Work items come from eight per-XCD queues (item j belongs to XCD j % 8; block b is expected on XCD b % 8 -- for speed only):
    // one same-address device atomic retires in ~12 ns, 24 576 of them on ONE counter were a 290 us floor for an 8-frame launch
    // (measured: 321 -> 243 us).  Queue position q of XCD x is item x + 8 q; a workgroup's first TWO positions are static (its
    // rank r among the XCD's workgroups, then r + their number), later ones come from the XCD's counter one patch ahead.
    const int xcd = blockIdx.x & 7;
    const int wgs_of_xcd = ((int)gridDim.x - xcd + 7) >> 3;
    int *ctr = work_counter + 256 + xcd * 32;   // ws + 1024 bytes: eight counters, one 128-byte line each (conv3 zeroes them)
    int j = xcd + 8 * (int)(blockIdx.x >> 3);
    int jn = j + 8 * wgs_of_xcd;                // the item after j
    int patch = 0, patch_next = 0;
    unsigned int row = 0u;
    if (j < n_items) {
        const unsigned long long *src;
        s1x_item(in, it, j, src, patch);
        patch = __builtin_amdgcn_readfirstlane(patch);
        row = ((const unsigned short *)src)[tid];
    }
    __syncthreads();
    const int row_slot = ((tid >> 4) + 1) * S1X_RP + (tid & 15) + 1;
    L.rows[0][row_slot] = row << 1;
    {
        const unsigned long long nzb = __ballot(row != 0u);  // 16 lanes per x row
        if (lane == 0)
            L.planes[0][wave] = ((nzb & 0xFFFFull) ? 1u : 0u) | ((nzb & 0xFFFF0000ull) ? 2u : 0u) | ((nzb & 0xFFFF00000000ull) ? 4u : 0u) |
                                ((nzb >> 48) ? 8u : 0u);
    }
    int rbuf = 0, cb = 0;  // rows buffer / cell-list buffer of the current patch
    int nprev = 0;         // cells of the previous patch still to be wiped from D
    int iter = 0;
    __syncthreads();
    unsigned int planes = L.planes[0][0] | (L.planes[0][1] << 4) | (L.planes[0][2] << 8) | (L.planes[0][3] << 12);  // bit x: row x holds a voxel
#ifdef CAELO_ENC_PROF
    if (tid < 16) L.prof[tid] = 0u;
    __syncthreads();
    unsigned s1x_t_prev = (unsigned)clock64();
#endif
    while (j < n_items) {
        // ---- phase B: request the next patch's rows and the item after it; wipe the previous patch's D entries; masks of
        // this patch's cells (GATHERED from the 4 x 4 voxel rows that feed a cell); queue the non-empty ones
        unsigned int row_next = 0u;
        if (jn < n_items) {
            const unsigned long long *src;
            s1x_item(in, it, jn, src, patch_next);
            patch_next = __builtin_amdgcn_readfirstlane(patch_next);
            row_next = ((const unsigned short *)src)[tid];
        }
        int j_fetch;   // defined and read in thread 0 only
        if (tid == 0) j_fetch = atomicAdd(ctr, 1);
        int wipe_i = tid;
        asm volatile("" : "+v"(wipe_i));   // (keeps hipcc from carrying this loop's LDS address across the patch loop in a spilled register)
        for (int i = wipe_i; i < nprev; i += 256) {
            const int cell = L.lcell[cb ^ 1][i];
            const int q = ((cell >> 6) * 10 + ((cell >> 3) & 7) + 1) * 10 + (cell & 7) + 1;
            L.d[2 * q] = make_uint4(0u, 0u, 0u, 0u);
            L.d[2 * q + 1] = make_uint4(0u, 0u, 0u, 0u);
        }
        unsigned long long cmask[2];
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
            const int px = wave + 4 * rep;  // wave-uniform; x rows 2px-1 .. 2px+2 feed the cells of this x plane
            const unsigned int need = (0xFu << (2 * px)) >> 1;
            cmask[rep] = 0ull;
            if (planes & need) {
                const int py = (tid >> 3) & 7, sh = 2 * (tid & 7);
                const unsigned int *rp = &L.rows[rbuf][(2 * px) * S1X_RP + 2 * py];
                unsigned int m32[2] = {0u, 0u};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const uint2 w01 = *(const uint2 *)(rp + a * S1X_RP), w23 = *(const uint2 *)(rp + a * S1X_RP + 2);
                    unsigned int acc = (w01.x >> sh) & 0xFu;
                    acc |= ((w01.y >> sh) & 0xFu) << 4;
                    acc |= ((w23.x >> sh) & 0xFu) << 8;
                    acc |= ((w23.y >> sh) & 0xFu) << 12;
                    m32[a >> 1] |= acc << ((a & 1) * 16);
                }
                cmask[rep] = (unsigned long long)m32[0] | ((unsigned long long)m32[1] << 32);
            }
        }
        {
            const unsigned long long bal0 = __ballot(cmask[0] != 0ull), bal1 = __ballot(cmask[1] != 0ull);
            const int c0n = __popcll(bal0), c1n = __popcll(bal1);
            if (c0n + c1n) {   // one LDS counter bump per wave for both x planes
                int base = 0;
                if (lane == 0) base = atomicAdd(&L.list_n[cb], c0n + c1n);
                base = __builtin_amdgcn_readfirstlane(base);
                // (lanes below this one: mbcnt -- a (1 << lane) - 1 mask is four registers the compiler keeps across the patch loop)
                if (cmask[0] != 0ull) {
                    const int slot = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal0, 0u));
                    L.lcell[cb][slot] = (unsigned short)tid;
                    L.lmask[slot] = cmask[0];
                }
                if (cmask[1] != 0ull) {
                    const int slot = base + c0n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal1, 0u));
                    L.lcell[cb][slot] = (unsigned short)(tid + 256);
                    L.lmask[slot] = cmask[1];
                }
            }
            if (lane < 2) {  // any lane of each byte (= y row of cells) -> bit 0 of the byte -> 8 bits
                unsigned long long t = lane ? bal1 : bal0;
                t |= t >> 4; t |= t >> 2; t |= t >> 1;
                L.nzrow[wave + 4 * lane + 1] = (unsigned int)(((t & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) << 1;
            }
        }
        S1X_STAMP(0);
        caelo_lds_barrier();
        S1X_STAMP(1);
        // ---- phase C: conv1 + pool1 + tanh of the queued cells, 16 per MFMA tile.  Everything the first tile needs is
        // requested at once (the list length arrives with it: slots past the end are discarded afterwards)
        const int nlist = L.list_n[cb];
        for (int tile = wave; tile == wave || tile * 16 < nlist; tile += 4) {
            const int slot = tile * 16 + n;
            unsigned long long mask = L.lmask[slot & 511];
            const bool upper = (n & 8) != 0;
            const int cs0 = tile * 16 + 4 * g + (upper ? 2 : 0);
            const int cell0 = L.lcell[cb][cs0 & 511], cell1 = L.lcell[cb][(cs0 + 1) & 511];
            uint4 wfr[8];   // the B fragments of one k step at a time (all sixteen were 64 registers: the kernel now lives on 168)
#pragma unroll
            for (int i = 0; i < 8; ++i) wfr[i] = L.wf[i][lane];
            if (tile * 16 >= nlist) break;
            if (slot >= nlist) mask = 0ull;
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks == 1)
#pragma unroll
                    for (int i = 0; i < 8; ++i) wfr[i] = L.wf[8 + i][lane];
                const unsigned int byte = ((unsigned int)(mask >> (32 * ks)) >> (8 * g)) & 0xFFu;
                uint4 a;  // bits 2i, 2i+1 -> halves 0x3C00 (1.0) / 0
                a.x = (((byte & 3u) * 0x8001u) & 0x10001u) * 0x3C00u;
                a.y = ((((byte >> 2) & 3u) * 0x8001u) & 0x10001u) * 0x3C00u;
                a.z = ((((byte >> 4) & 3u) * 0x8001u) & 0x10001u) * 0x3C00u;
                a.w = ((((byte >> 6) & 3u) * 0x8001u) & 0x10001u) * 0x3C00u;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[nt] = S1X_MFMA(a, wfr[nt * 2 + 1], acc[nt]);  // low terms first
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[nt] = S1X_MFMA(a, wfr[nt * 2], acc[nt]);
            }
            if (COUNT) n_mfma = (unsigned)__builtin_amdgcn_readfirstlane((int)(n_mfma + 16u));   // (wave-uniform: a scalar register)
            // C rows 4g + r = cells of the tile, column n = (sub-position parity, channel) of n-tile nt = sub-positions 2nt, 2nt+1:
            // max over the 8 sub-positions = over nt in registers and over n <-> n ^ 8 by one DPP rotate (tanh is monotone)
            float pooled[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float m = fmaxf(fmaxf(acc[0][r], acc[1][r]), fmaxf(acc[2][r], acc[3][r]));
                pooled[r] = fmaxf(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x128, 0xF, 0xF, true)));  // row_ror:8
            }
            // lanes n < 8 finish cells 4g, 4g+1, lanes n >= 8 cells 4g+2, 4g+3 (channel n & 7).  (Selected as VALUES: written
            // `upper ? pooled[2 + rr] : pooled[rr]` hipcc selects the ADDRESS and sends the array to LDS, 4 KB and three trips per tile.)
            const float p0_ = pooled[0], p1_ = pooled[1], p2_ = pooled[2], p3_ = pooled[3];
            const float pick[2] = {upper ? p2_ : p0_, upper ? p3_ : p1_};
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const float v = pick[rr];
                if (cs0 + rr < nlist) {
                    const int cell = rr ? cell1 : cell0;
                    const int yp = ((cell >> 3) & 7) + 1;
                    const int q = ((cell >> 6) * 10 + yp) * 10 + (cell & 7) + 1;
                    const float dv = enc_act<H>(v + b1c) - bgc;
                    const _Float16 hi = (_Float16)dv;
                    const _Float16 lo = (_Float16)(dv - (float)hi);
                    _Float16 *du = (_Float16 *)&L.d[2 * q];   // units: d_hi x 8 channels, d_lo x 8 channels; swapped in odd padded-y rows
                    du[8 * (yp & 1) + (n & 7)] = hi;
                    du[8 * ((yp & 1) ^ 1) + (n & 7)] = lo;
                }
            }
        }
        S1X_STAMP(2);
        caelo_lds_barrier();
        S1X_STAMP(3);
        // ---- phase D: conv2 (8 -> 16) + pool2 + tanh; per row pair yi this wave owns the x pair xp = wave ^ d(yi)
        float2 pout[4];  // this lane's two pooled outputs of each pair (stored after the loop)
        // The lane constants of this phase are formed HERE, from a lane index hipcc cannot see through: everything derived from
        // threadIdx is loop invariant, so left alone the compiler computes ~40 per-lane addresses once, keeps them across all
        // three phases of the patch loop and spills what does not fit in 168 registers (round 3 had 253 to burn).
        int ln_ = lane;
        asm volatile("" : "+v"(ln_));
        const int g_ = ln_ >> 4, n_ = ln_ & 15;
    // lane constants of the conv2 A operand: row m = n -> (yl, z); k group g -> (z tap, term) per fragment; the unit of a term is
    // swapped in odd padded-y rows: a slab whose first row is even (kb even) uses the E pointers, an odd one the O pointers
    const int lyl = s1x_yl(n_ >> 2);
    const int lq = lyl * 10 + 4 * s1x_zh(n_ >> 2) + (n_ & 3);   // position of A row m = n for z tap 0 (zp = z + tap)
    const int t0_ = g_ == 3 ? 0 : g_, t2_ = 1 + (g_ & 1), u2_ = g_ >> 1;
    const int iA0 = 2 * (lq + t0_) + (0 ^ lyl);     // uint4 indices into d for even rows; an odd first row flips the unit: index ^ 1
    const int iA1 = 2 * (lq + t0_) + (1 ^ lyl);     // (every offset added below is even)
    const int iA2 = 2 * (lq + t2_) + (u2_ ^ lyl);
    // this lane's C rows 4g + r = (yl, z = 4 zh + r): the border class of z per r is fixed, that of y depends on the pair's yi
    const int gyl = s1x_yl(g_), gzh = s1x_zh(g_);
        {
            // ONE scalar mask of the active slabs of all four pairs, bit yi * 12 + plane * 3 + kb: lane b < 48 looks its bit up (one LDS
            // word: the occupied rows of its plane) and a ballot collects them.  (Round 3 read the sixteen words in every lane, moved
            // each through readfirstlane and assembled the mask with ~160 scalar instructions per patch and wavefront: the per-item
            // overhead of this kernel is its instruction count -- an EMPTY patch cost 190 scalar + 150 vector instructions per wavefront.)
            unsigned long long act;
            {
                const int yi_ = ln_ / 12, pp_ = (ln_ % 12) / 3, kb_ = ln_ % 3;
                const int xd_ = (0x2130 >> (4 * (yi_ & 3))) & 3;                    // S1_XDEAL: 0, 3, 1, 2
                const unsigned int nz = L.nzrow[(2 * (wave ^ xd_) + pp_) % 12];
                act = __ballot(ln_ < 48 && ((nz >> (2 * yi_ + kb_)) & 3u) != 0u);
            }
#pragma unroll
            for (int yi = 0; yi < 4; ++yi) {
                const int xp = wave ^ S1_XDEAL(yi);
                const unsigned int pact = (unsigned int)(act >> (12 * yi)) & 0xFFFu;
                if (pact == 0u) {  // nothing but background feeds this pair: per-model constants, needed only when the patch is stored
                    pout[yi] = bgo[yi];
                    continue;
                }
                // C0 of the pair's two tiles (x = 2xp, 2xp + 1; rows y = 2yi + yl, z = 4zh + r) from the class table: two LDS words per tile
                f32x4 acc0a, acc1a;
                {
                    const int y_ = 2 * yi + gyl;
                    const int cy = y_ == 0 ? 0 : (y_ == 7 ? 2 : 1);
#pragma unroll
                    for (int xt = 0; xt < 2; ++xt) {
                        const int x_ = 2 * xp + xt;
                        const int cx = x_ == 0 ? 0 : (x_ == 7 ? 2 : 1);
                        const float ci = L.c0cls[(cx * 3 + cy) * 3 + 1][n_], ce = L.c0cls[(cx * 3 + cy) * 3 + (gzh ? 2 : 0)][n_];
                        const f32x4 c = {gzh ? ci : ce, ci, ci, gzh ? ce : ci};
                        if (xt == 0) acc0a = c; else acc1a = c;
                    }
                }
                f32x4 acc0b = {0.f, 0.f, 0.f, 0.f}, acc1b = {0.f, 0.f, 0.f, 0.f};
                {
                // slab k = plane * 3 + kb of the pair's four input planes 2xp - 1 .. 2xp + 2 (a plane outside the patch is never active).
                // PLANE BY PLANE (round 4): the nine fragments of an ACTIVE plane are requested together, unconditionally within the plane
                // (straight-line loads: hipcc counts the waits, lgkmcnt(6) / (3) / (0)), and a plane with no active slab is skipped, loads
                // and all.  Round 3 fetched all 36 fragments of an active pair through a three-slab ring: one LDS round trip per pair
                // instead of one per active plane, but ~60 % of those reads fed no MFMA and the LDS is this kernel's most loaded unit
                // (201 -> 194 us per 24 576 patches; conditional loads per SLAB spill -- 160 B of scratch -- and take 306 us).
                // The lane bases of the pair are formed HERE from one scalar (left to itself hipcc hoists the 144 per-slab addresses of
                // the four pairs out of the patch loop and spills them); slab offsets are instruction immediates.
                int po = 2 * (((2 * xp - 1) * 10 + 2 * yi) * 10);
                asm volatile("" : "+s"(po));
                const int b0 = iA0 + po, b1 = iA1 + po, b2 = iA2 + po;
                uint4 fr[3][3];
#define S1X_LOAD(K)                                                           \
    {                                                                         \
        const int o_ = 2 * (((K) / 3) * 100 + ((K) % 3) * 10);                \
        fr[(K) % 3][0] = L.d[((K) % 3 == 1 ? (b0 ^ 1) : b0) + o_];     \
        fr[(K) % 3][1] = L.d[((K) % 3 == 1 ? (b1 ^ 1) : b1) + o_];     \
        fr[(K) % 3][2] = L.d[((K) % 3 == 1 ? (b2 ^ 1) : b2) + o_];     \
    }
#pragma unroll
                for (int P = 0; P < 4; ++P) {
                    const unsigned int pl = (pact >> (3 * P)) & 7u;
                    if (pl == 0u) continue;
#pragma unroll
                    for (int KB = 0; KB < 3; ++KB) S1X_LOAD(3 * P + KB)
#pragma unroll
                    for (int KB = 0; KB < 3; ++KB) {
                        if ((pl >> KB) & 1u) {
                            const int k = 3 * P + KB;
                            const uint4 a0 = fr[k % 3][0], a1 = fr[k % 3][1], a2 = fr[k % 3][2];
                            if (P <= 2) acc0a = S1X_MFMA(a0, bq[(P <= 2 ? P : 0) * 3 + KB][0], acc0a);
                            if (P >= 1) acc1a = S1X_MFMA(a0, bq[(P >= 1 ? P - 1 : 0) * 3 + KB][0], acc1a);
                            if (P <= 2) acc0b = S1X_MFMA(a1, bq[(P <= 2 ? P : 0) * 3 + KB][0], acc0b);
                            if (P >= 1) acc1b = S1X_MFMA(a1, bq[(P >= 1 ? P - 1 : 0) * 3 + KB][0], acc1b);
                            if (P <= 2) acc0b = S1X_MFMA(a2, bq[(P <= 2 ? P : 0) * 3 + KB][1], acc0b);
                            if (P >= 1) acc1b = S1X_MFMA(a2, bq[(P >= 1 ? P - 1 : 0) * 3 + KB][1], acc1b);
                            if (COUNT) n_mfma = (unsigned)__builtin_amdgcn_readfirstlane((int)(n_mfma + (P <= 2 ? 3u : 0u) + (P >= 1 ? 3u : 0u)));
                        }
                    }
                }
                acc0a += acc0b;
                acc1a += acc1b;
                }
                // ---- pool2: x pair in registers, z pairs in registers, y pair across lane groups g <-> g ^ 1 (v_permlane16_swap)
                float v0 = fmaxf(fmaxf(acc0a[0], acc0a[1]), fmaxf(acc1a[0], acc1a[1]));
                float v1 = fmaxf(fmaxf(acc0a[2], acc0a[3]), fmaxf(acc1a[2], acc1a[3]));
                const auto s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v0), __float_as_uint(v0), false, false);
                const auto s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v1), __float_as_uint(v1), false, false);
                v0 = fmaxf(__uint_as_float(s0[0]), __uint_as_float(s0[1]));
                v1 = fmaxf(__uint_as_float(s1[0]), __uint_as_float(s1[1]));
                pout[yi] = make_float2(enc_act<H>(v0), enc_act<H>(v1));
            }
        }
        S1X_STAMP(8);
#ifdef CAELO_ENC_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (profiling build only: slot 11 = everything this wavefront had outstanding in memory is back)
        S1X_STAMP(11);
#endif
        // ---- the next patch's rows and the item after it, requested at the top of phase B, are taken up HERE, at the end of the
        // patch: a memory-side atomic and an HBM load take ~2 us to return under this kernel's load, and here they have had the
        // whole patch.  (They used to be waited for before conv2; moving the wait changed nothing measurable -- 233 us per
        // 24 576 patches either way, 105 us for empty patches -- so that wait was not what the two waves of a SIMD stood on.)
        // The P2 stores of this patch go out after the wait (vmcnt counts stores too: issued before it, the wait would drain them).
        L.rows[rbuf ^ 1][row_slot] = row_next << 1;
        {
            const unsigned long long nzb = __ballot(row_next != 0u);
            if (lane == 0)
                L.planes[rbuf ^ 1][wave] = ((nzb & 0xFFFFull) ? 1u : 0u) | ((nzb & 0xFFFF0000ull) ? 2u : 0u) |
                                           ((nzb & 0xFFFF00000000ull) ? 4u : 0u) | ((nzb >> 48) ? 8u : 0u);
        }
        if (tid == 0) {
            L.next_j[iter & 1] = xcd + 8 * (2 * wgs_of_xcd + j_fetch);
            L.list_n[cb ^ 1] = 0;  // the list wiped in this iteration's phase B becomes the next patch's
        }
        S1X_STAMP(9);
#ifndef S1X_NOSTORE
        if (!(g_ & 1)) {
            unsigned lane_off = (unsigned)(32 * gzh + n_) * 4u;   // bytes; pooled z = 2 (z >> 2) + {0, 1}, channel n: ONE lane register for the four pairs
            asm volatile("" : "+v"(lane_off));                  // (formed here, not carried across the patch loop)
#pragma unroll
            for (int yi = 0; yi < 4; ++yi) {
                const int xp = wave ^ S1_XDEAL(yi);
                char *dst = (char *)(p2out + (size_t)patch * 1024 + (size_t)((xp * 4 + yi) * 64));   // (wave-uniform base, 32-bit lane offset)
                *(float *)(dst + lane_off) = pout[yi].x;
                *(float *)(dst + lane_off + 64u) = pout[yi].y;
            }
        }
#else
        if (pout[0].x + pout[1].x + pout[2].x + pout[3].x == 12345.678f) p2out[0] = pout[0].y;
#endif
        S1X_STAMP(10);
        nprev = nlist;
        j = jn;
        patch = patch_next;
        rbuf ^= 1;
        cb ^= 1;
        ++iter;
        S1X_STAMP(4);
#ifdef CAELO_ENC_PROF
        if (threadIdx.x == 0) { L.prof[6] += 1; L.prof[7] += nprev; }
#endif
        caelo_lds_barrier();
        S1X_STAMP(5);
        jn = __builtin_amdgcn_readfirstlane(L.next_j[(iter - 1) & 1]);
        planes = L.planes[rbuf][0] | (L.planes[rbuf][1] << 4) | (L.planes[rbuf][2] << 8) | (L.planes[rbuf][3] << 12);
    }
#ifdef CAELO_ENC_PROF
    if (threadIdx.x == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&g_enc_stamp[i], (unsigned long long)L.prof[i]);
#endif
    if (COUNT) {
        // (the count is the wavefront's: every lane holds it.)  One atomic per WORKGROUP, on one of eight 128-byte lines: round 3 .. 6 ended
        // every wavefront with an atomic on ONE word -- 3 072 same-address atomics at ~12 ns each, a tail of up to 37 us that only the
        // profiling launches (bench.py's roofline, tools/roofline_launch.py) paid: tools/s1x_probe_n.sh, profiles/r06_s1x_ablation.txt
        __syncthreads();
        if (tid == 0) L.list_n[0] = 0;
        __syncthreads();
        if (lane == 0) atomicAdd(&L.list_n[0], (int)n_mfma);
        __syncthreads();
        if (tid == 0) atomicAdd(mfma_count + 16 * (blockIdx.x & 7), (unsigned long long)(unsigned)L.list_n[0]);
    }
}
#define ENC_STAGE1X_ARGS const caelo_enc_in in, int64_t n_patches, int group, int *__restrict__ work_counter,                     \
                         const uint4 *__restrict__ w1f, const float *__restrict__ b1g, const uint4 *__restrict__ w2x,             \
                         const float *__restrict__ c0g, float *__restrict__ p2out, unsigned long long *__restrict__ mfma_count
template <bool COUNT>
__global__ void __launch_bounds__(256, 3) k_enc_stage1x(ENC_STAGE1X_ARGS) {
    enc_stage1x_body<CAELO_ACT_TANH, COUNT>(in, n_patches, group, work_counter, w1f, b1g, w2x, c0g, p2out, mfma_count);
}
template <bool COUNT>
__global__ void __launch_bounds__(256, 3) k_enc_stage1x_relu(ENC_STAGE1X_ARGS) {
    enc_stage1x_body<CAELO_ACT_RELU, COUNT>(in, n_patches, group, work_counter, w1f, b1g, w2x, c0g, p2out, mfma_count);
}
