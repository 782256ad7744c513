// enc_stage1.inc -- k_enc_stage1, the exact-f32 stage 1 (conv1 + pool1 + conv2 + pool2); part of encoder.hip.  The PRECISION
// REFERENCE of the f16 x 2 k_enc_stage1x (enc_stage1x.inc): a context runs it after caelo_set_encoder_reference(c, 1).
//
// conv1 + pool1 (VALU, sparse) -> conv2 (v_mfma_f32_16x16x4_f32, all 54 B fragments of W2 resident in VGPRs, sparse over
// background) -> pool2 in registers (act(max) == max(act)) -> P2 [patch][4][4][4][16].  Persistent workgroups, one patch at a time
// from a global work counter, coarsest scale first.
//
// A voxel patch is mostly empty (2 / 54 / 67 set voxels of 4096 at the three scales), so after
// conv1+pool1 most of the 8^3 cells hold the constant background vector bg = tanh(b1).  conv2 is
// linear before its tanh:  conv2(P1) = conv2(BG) + conv2(P1 - BG),  BG = bg in every valid cell.
//   * C0 = b2 + conv2(BG) is a [512][16] table computed once per model (host, at weight load);
//   * D = P1 - BG is zero except in the few cells whose 4^3 receptive field holds a set voxel.
// The kernel keeps D in LDS (two 4-channel planes with a 1-cell halo), starts every MFMA accumulator
// from C0 and skips -- exactly, a skipped product is an added zero -- every (m-tile, x-tap plane)
// whose 4 x 8 input rows are all-zero in D: 71 % of the conv2 MFMAs on KITTI-shaped scans.
//
// D layout: channel half p, padded position q (0..999), channel c:
//   D[p*S1P_PLANE + q*4 + c],   q = (xp*10 + yp)*10 + zp,  xp, yp, zp in 0..9 (1-cell halo on every axis, zp = z + 1):
// the two out-of-range z taps read stored zeros, nothing is predicated.
#ifdef CAELO_ENC_PROF  // make PROF=1: slots 0..5 accumulate shader-clock cycles per phase over all patches, 6 = patches, 7 = queued cells.
// Caveat: s_memtime drains the wave's outstanding stores first, so the phase that ends with the P2 stores ("conv2")
// is inflated by their latency; use tools/enc_scale_prof.py (unprofiled build) for absolute numbers.
#define ENC_STAMP(i) do { if (threadIdx.x == 0) { const unsigned t_ = (unsigned)clock64(); L.prof[i] += t_ - enc_t_prev; enc_t_prev = t_; } } while (0)
#else
#define ENC_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0 && patch == 0) g_enc_stamp[i] = wall_clock64(); } while (0)
#endif
#define S1P_PLANE ((1000 + 4) * 4)   // floats per 4-channel half, +4 cells: the two halves start 16 banks apart
#define S1_RPITCH 20
#define S1_ROWS (18 * S1_RPITCH)
struct Stage1Lds {
    float p1[2 * S1P_PLANE];
    float w1[27 * 8];
    float b1[8];
    float bg[8];
    unsigned long long cell_mask[512];  // per pooled cell: set voxels of its 4^3 receptive field, bit a*16 + b*4 + j
    unsigned short list_cell[512];      // the cells with a non-zero mask, in arrival order
    unsigned int nzrow[12];  // per padded xp: bit yp set when some cell (xp, yp, *) is non-background
    float2 bgout[4][4][32];  // [wave][yi][lane < 32]: outputs of a tile pair that sees nothing but background (see the kernel)
    unsigned short rows[2][S1_ROWS];  // the patch's 256 voxel rows (16 z bits each) with a zero border: [x + 1][y + 1], pitch S1_RPITCH
    int list_n;
    int next_j;
#ifdef CAELO_ENC_PROF
    unsigned int prof[8];
#endif
};

// 3 taps (one (ka, kb) pair of input rows) of one m-tile: 6 MFMAs on two interleaved accumulators
#define CONV2Z_ROW(ACC_A, ACC_B, APTR, KA, KB)                                                     \
    _Pragma("unroll") for (int kc = 0; kc < 3; ++kc) {                                             \
        const int t = (KA) * 9 + (KB) * 3 + kc;                                                     \
        const float2 av = *(const float2 *)((APTR) + (((KA) * 10 + (KB)) * 10 + (kc - 1)) * 4);     \
        ACC_A = MFMA16(av.x, breg[t][0], ACC_A);                                                    \
        ACC_B = MFMA16(av.y, breg[t][1], ACC_B);                                                    \
    }
// all 9 (ka, kb) row pairs of one tile; NZk = occupancy bits of padded plane x + k, shifted down by y0:
// tap row kb reads input rows y0 + kb and y0 + kb + 1
#define CONV2Z_TILE(ACC_A, ACC_B, APTR, NZ0, NZ1, NZ2)                                              \
    if ((NZ0) & 0x3u) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 0, 0) }                                      \
    if ((NZ0) & 0x6u) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 0, 1) }                                      \
    if ((NZ0) & 0xCu) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 0, 2) }                                      \
    if ((NZ1) & 0x3u) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 1, 0) }                                      \
    if ((NZ1) & 0x6u) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 1, 1) }                                      \
    if ((NZ1) & 0xCu) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 1, 2) }                                      \
    if ((NZ2) & 0x3u) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 2, 0) }                                      \
    if ((NZ2) & 0x6u) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 2, 1) }                                      \
    if ((NZ2) & 0xCu) { CONV2Z_ROW(ACC_A, ACC_B, APTR, 2, 2) }
// (the body of k_enc_stage1 and of its relu sibling: H = the hidden activation)
template <int H>
static __device__ __forceinline__ void enc_stage1_body(const caelo_enc_in &in, int64_t n_patches,
                                                       int group, int *__restrict__ work_counter,
                                                       const float *__restrict__ w1g, const float *__restrict__ b1g,
                                                       const float *__restrict__ w2g, const float *__restrict__ c0g,
                                                       float *__restrict__ p2out) {
    __shared__ __attribute__((aligned(16))) Stage1Lds L;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane >> 4;   // MFMA k-group
    const int n = lane & 15;   // MFMA column (output channel) for B/C, row for A
    // ---- one-time: weights.  B fragment for k-step (tap t, h): W2[t][cin = 2g + h][n]
    float breg[27][2];
#pragma unroll
    for (int t = 0; t < 27; ++t) {
        breg[t][0] = w2g[(t * 8 + 2 * g) * 16 + n];
        breg[t][1] = w2g[(t * 8 + 2 * g + 1) * 16 + n];
    }
    // Tile pairs are dealt to the 4 waves as a XOR Latin square: wave w owns, for every row pair yi, the x pair xp = w ^ d(yi),
    // d = 0, 3, 1, 2 -- every 2x2 cluster of occupied pairs lands on 4 different waves, and of all 24^3 ways to give each wave one
    // pair per yi this one balances the MFMA rows best on the golden frames (tools/conv2_balance.py: average / busiest wavefront
    // 0.83; round 1's xp = (w - 2 yi) mod 4: 0.78; the worst deal: 0.58).
    // C0 = b2 + conv2(BG) accumulator fragments of this lane's 8 m-tiles are patch independent: loaded once,
    // together with the outputs tanh(pool2(C0)) of a pair that sees nothing but background.
    // (the all-background outputs live in LDS, not in registers: with them the kernel spilled 5 registers, and every reload
    // on the background path -- a scratch load followed by s_waitcnt vmcnt(0) -- also waited for the P2 stores before it)
    f32x4 c0r[4][2];
#pragma unroll
    for (int yi = 0; yi < 4; ++yi) {
        const int xp = wave ^ S1_XDEAL(yi);
#pragma unroll
        for (int xt = 0; xt < 2; ++xt) {
            const float *c0a = c0g + (size_t)((((2 * xp + xt) * 8 + 2 * yi + (g >> 1)) * 8 + 4 * (g & 1)) * 16 + n);
            c0r[yi][xt] = (f32x4){c0a[0], c0a[16], c0a[32], c0a[48]};
        }
        float v0 = fmaxf(fmaxf(c0r[yi][0][0], c0r[yi][0][1]), fmaxf(c0r[yi][1][0], c0r[yi][1][1]));
        float v1 = fmaxf(fmaxf(c0r[yi][0][2], c0r[yi][0][3]), fmaxf(c0r[yi][1][2], c0r[yi][1][3]));
        v0 = fmaxf(v0, __shfl_xor(v0, 32));
        v1 = fmaxf(v1, __shfl_xor(v1, 32));
        if (lane < 32) L.bgout[wave][yi][lane] = make_float2(enc_act<H>(v0), enc_act<H>(v1));
    }
    for (int i = tid; i < 27 * 8; i += 256) L.w1[i] = w1g[i];
    if (tid < 8) { L.b1[tid] = b1g[tid]; L.bg[tid] = c0g[512 * 16 + tid]; }  // bg = tanh(b1), from the host table
    for (int i = tid; i < 2 * S1P_PLANE; i += 256) L.p1[i] = 0.0f;  // D == 0: halo, pads, background cells
    for (int i = tid; i < 512; i += 256) L.cell_mask[i] = 0ull;
    for (int i = tid; i < 2 * S1_ROWS; i += 256) (&L.rows[0][0])[i] = 0;  // the border stays zero
    if (tid == 0) L.list_n = 0;
    if (tid < 12) L.nzrow[tid] = 0u;
    __syncthreads();
    const int n_items = enc_items_total(in, n_patches);  // distinct patches of the launch (all of them without de-duplication)

#ifdef CAELO_ENC_PROF
    unsigned enc_t_prev = (unsigned)clock64();  // phase totals accumulate in LDS (registers would spill at 3 workgroups/CU)
    if (tid < 8) L.prof[tid] = 0u;
    __syncthreads();
#endif
    // Patches cost ~1x / 1.5x / 2.5x at the three scales (set voxels 2 / 54 / 67).  Work item j -> scale
    // group-1 - j / nk, keypoint j % nk, i.e. coarsest scale first; a persistent workgroup takes the items
    // j = blockIdx.x + k * gridDim.x and so meets a mix of scales instead of one scale only.
    const int nk = (int)(n_patches / group);
    if (blockIdx.x == 0 && tid < 8) work_counter[C3X_TICKET_INT + 32 * tid] = 0;   // conv3 (the next kernel on this stream) draws its pairs from here
    int j = blockIdx.x;
    // thread = one 16-voxel row of the patch (ix = tid >> 4, iy = tid & 15, bit = iz); fetched one patch ahead
    unsigned int row = 0u;
    int patch = 0, patch_next = 0;  // output rows of the current / the prefetched item (wave-uniform)
    if (j < n_items) {
        const unsigned long long *src;
        enc_item(in, j, nk, group, src, patch);
        patch = __builtin_amdgcn_readfirstlane(patch);
        row = ((const unsigned short *)src)[tid];
    }
    const int row_slot = ((tid >> 4) + 1) * S1_RPITCH + (tid & 15) + 1;  // where this thread's row lives in L.rows[*]
    L.rows[0][row_slot] = (unsigned short)row;
    int rbuf = 0;
    __syncthreads();
    while (j < n_items) {
        ENC_STAMP(0);
        // work items beyond the first come from a global counter (patch costs vary 10x: a static split leaves the
        // average workgroup idle for the last ~55 us of the launch); fetched after the mask scatter, published
        // through LDS at the barrier that ends conv1, i.e. microseconds later

        // ---- B1: the receptive-field masks of this thread's two pooled cells (c and c + 256), GATHERED from the 4 x 4 voxel
        // rows that feed them: bit a*16 + b*4 + j <-> voxel (2px-1+a, 2py-1+b, 2pz-1+j).  Two aligned 32-bit LDS reads per
        // (cell, a) = rows y' = 2py .. 2py+3 of the bordered copy; no atomics, no barrier between mask building and queueing
        // (round 1 scattered every set voxel into up to 8 masks with LDS ORs: 1 500 wave instructions per patch, 5 barriers).
        unsigned long long cmask[2];
        {
            const int py = (tid >> 3) & 7, sh = 2 * (tid & 7);
#pragma unroll
            for (int rep = 0; rep < 2; ++rep) {
                const int px = (tid >> 6) + 4 * rep;
                const unsigned int *rp = (const unsigned int *)&L.rows[rbuf][(2 * px) * S1_RPITCH + 2 * py];  // x' = 2px + a, y' = 2py
                unsigned int m32[2] = {0u, 0u};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const unsigned int w0 = rp[a * (S1_RPITCH / 2)], w1 = rp[a * (S1_RPITCH / 2) + 1];
                    const unsigned int n0 = (((w0 & 0xFFFFu) << 1) >> sh) & 0xFu, n1 = (((w0 >> 16) << 1) >> sh) & 0xFu;
                    const unsigned int n2 = (((w1 & 0xFFFFu) << 1) >> sh) & 0xFu, n3 = (((w1 >> 16) << 1) >> sh) & 0xFu;
                    m32[a >> 1] |= (n0 | (n1 << 4) | (n2 << 8) | (n3 << 12)) << ((a & 1) * 16);
                }
                cmask[rep] = (unsigned long long)m32[0] | ((unsigned long long)m32[1] << 32);
            }
        }
        // issued here, after this patch's prefetched rows were consumed (vmcnt counts in order: an earlier wait for them
        // would also wait for the atomic); consumed at the end of conv1, microseconds later.  Tried and dropped: handing the items
        // out four per atomic (364 -> 348 us for an 8-frame launch, 64 -> 84 us for one frame), and fetching one patch AHEAD (the
        // round trip then never shows in the phase profile, but pinning a second item per workgroup costs balance: 359 -> 365 us
        // per 8-frame launch, 62 -> 66 us for one frame, 11.09 -> 11.03 k frames/s).
        int j_fetch;  // defined in thread 0 only, and only read there (no merge copy that would wait for the atomic)
        if (tid == 0) j_fetch = atomicAdd(work_counter, 1);
        ENC_STAMP(1);
        // ---- queue the cells with a non-empty mask (one LDS counter bump per wave)
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
            const int cell = tid + rep * 256;
            const bool hit = cmask[rep] != 0ull;
            const unsigned long long bal = __ballot(hit);
            if (bal != 0ull) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&L.list_n, __popcll(bal));
                base = __shfl(base, 0);
                if (hit) {
                    L.list_cell[base + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)cell;
                    L.cell_mask[cell] = cmask[rep];
                    atomicOr(&L.nzrow[(cell >> 6) + 1], 1u << (((cell >> 3) & 7) + 1));
                }
            }
        }
        caelo_lds_barrier();
        ENC_STAMP(2);
        const int nlist = L.list_n;
        // ---- B2: conv1 + pool1 + tanh on the queued cells; 8 lanes = the 8 positions of a pooling block
        for (int base = wave * 8; base < nlist; base += 32) {
            const int item = base + (lane >> 3);
            const int sub = lane & 7;
            float acc[8];
            int cell = 0;
            if (item < nlist) {
                cell = L.list_cell[item];
                const unsigned long long mask = L.cell_mask[cell];
                const int sa = sub >> 2, sb = (sub >> 1) & 1, sc = sub & 1;
                unsigned int taps = 0;  // bit (ka*3+kb)*3+kc
#pragma unroll
                for (int ka = 0; ka < 3; ++ka)
#pragma unroll
                    for (int kb = 0; kb < 3; ++kb)
                        taps |= ((unsigned int)(mask >> ((sa + ka) * 16 + (sb + kb) * 4 + sc)) & 7u) << ((ka * 3 + kb) * 3);
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = L.b1[c];
                while (taps) {  // ascending tap order == the oracle's (kx,ky,kz) order
                    const int t = __ffs((int)taps) - 1;
                    taps &= taps - 1;
                    const float4 wa = *(const float4 *)&L.w1[t * 8], wb = *(const float4 *)&L.w1[t * 8 + 4];
                    acc[0] += wa.x; acc[1] += wa.y; acc[2] += wa.z; acc[3] += wa.w;
                    acc[4] += wb.x; acc[5] += wb.y; acc[6] += wb.z; acc[7] += wb.w;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = -3.0e38f;
            }
            // max over the pooling block = 8 aligned lanes (tanh is monotone: pool the pre-activations); DPP
            // lane swaps (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror) instead of 24 ds_bpermute round trips
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                acc[c] = fmaxf(acc[c], __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[c]), 0xB1, 0xF, 0xF, true)));
                acc[c] = fmaxf(acc[c], __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[c]), 0x4E, 0xF, 0xF, true)));
                acc[c] = fmaxf(acc[c], __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc[c]), 0x141, 0xF, 0xF, true)));
            }
            if (item < nlist) {
                float mine = acc[0];  // lane `sub` finishes channel `sub`
#pragma unroll
                for (int c = 1; c < 8; ++c) mine = (sub == c) ? acc[c] : mine;
                const int px = cell >> 6, py = (cell >> 3) & 7, pz = cell & 7;
                const int q = ((px + 1) * 10 + (py + 1)) * 10 + pz + 1;
                L.p1[(sub >> 2) * S1P_PLANE + q * 4 + (sub & 3)] = enc_act<H>(mine) - L.bg[sub];
            }
        }
        if (tid == 0) L.next_j = (int)gridDim.x + j_fetch;
        caelo_lds_barrier();
        ENC_STAMP(3);
        const int jn = __builtin_amdgcn_readfirstlane(L.next_j);
        unsigned int row_next = 0u;
        if (jn < n_items) {
            const unsigned long long *src;
            enc_item(in, jn, nk, group, src, patch_next);
            patch_next = __builtin_amdgcn_readfirstlane(patch_next);
            row_next = ((const unsigned short *)src)[tid];
        }
        // ---- conv2 (8->16) on MFMA: per row pair yi this wave owns the x pair xp = wave ^ d(yi)
        {
            const int yl = n >> 3, z = n & 7;  // A row m = yl*8 + z
            const float *plane = L.p1 + (g >> 1) * S1P_PLANE + 2 * (g & 1);
#pragma unroll
            for (int yi = 0; yi < 4; ++yi) {
                const int y0 = 2 * yi;
                const int xp = wave ^ S1_XDEAL(yi);
                // wave-uniform occupancy of the input rows yp = y0 .. y0+3 in the padded planes 2xp .. 2xp+3
                const unsigned int r0 = (unsigned)__builtin_amdgcn_readfirstlane((int)((L.nzrow[2 * xp] >> y0) & 0xFu));
                const unsigned int r1 = (unsigned)__builtin_amdgcn_readfirstlane((int)((L.nzrow[2 * xp + 1] >> y0) & 0xFu));
                const unsigned int r2 = (unsigned)__builtin_amdgcn_readfirstlane((int)((L.nzrow[2 * xp + 2] >> y0) & 0xFu));
                const unsigned int r3 = (unsigned)__builtin_amdgcn_readfirstlane((int)((L.nzrow[2 * xp + 3] >> y0) & 0xFu));
                // C column = n (channel), rows 4g..4g+3 -> z = 4*(g&1)+r ; pooled cell (xp, yi, 2*(g&1)+{0,1})
                float *dst = p2out + (size_t)patch * 1024 + (size_t)(((xp * 4 + yi) * 4 + 2 * (g & 1)) * 16 + n);
                if ((r0 | r1 | r2 | r3) == 0u) {  // nothing but background feeds this pair: per-model constants
                    if (g < 2) {
                        const float2 o = L.bgout[wave][yi][lane];
                        dst[0] = o.x; dst[16] = o.y;
                    }
                    continue;
                }
                // accumulators start from C0 = b2 + conv2(BG); two per tile to keep the MFMA chains independent
                f32x4 acc0 = c0r[yi][0];
                f32x4 acc1 = c0r[yi][1];
                f32x4 acc0b = {0.f, 0.f, 0.f, 0.f}, acc1b = {0.f, 0.f, 0.f, 0.f};
                // padded position of (x = 2xp, y = y0 + yl, z) for tap (0,0,1): xp' = x + ka, yp = y + kb
                const int qbase = ((2 * xp) * 10 + (y0 + yl)) * 10 + z + 1;
                const float *a0 = plane + qbase * 4;
                const float *a1 = a0 + 100 * 4;
                CONV2Z_TILE(acc0, acc0b, a0, r0, r1, r2)
                CONV2Z_TILE(acc1, acc1b, a1, r1, r2, r3)
                acc0 += acc0b;
                acc1 += acc1b;
                // ---- pool2: x pair in registers, z pairs in registers, y pair across lanes g <-> g^2
                float v0 = fmaxf(fmaxf(acc0[0], acc0[1]), fmaxf(acc1[0], acc1[1]));  // pz = 2*(g&1)
                float v1 = fmaxf(fmaxf(acc0[2], acc0[3]), fmaxf(acc1[2], acc1[3]));  // pz = 2*(g&1)+1
                v0 = fmaxf(v0, __shfl_xor(v0, 32));
                v1 = fmaxf(v1, __shfl_xor(v1, 32));
                if (g < 2) {
                    dst[0] = enc_act<H>(v0);
                    dst[16] = enc_act<H>(v1);
                }
            }
        }
        caelo_lds_barrier();
        ENC_STAMP(4);
#ifdef CAELO_ENC_PROF
        if (threadIdx.x == 0) { L.prof[6] += 1; L.prof[7] += nlist; }
#else
        if (threadIdx.x == 0 && blockIdx.x == 0 && patch == 0) g_enc_stamp[8] = (unsigned long long)nlist;
#endif
        // ---- back to D == 0 for the next patch
        for (int i = tid; i < nlist * 2; i += 256) {
            const int cell = L.list_cell[i >> 1];
            const int px = cell >> 6, py = (cell >> 3) & 7, pz = cell & 7;
            const int q = ((px + 1) * 10 + (py + 1)) * 10 + pz + 1;
            *(float4 *)&L.p1[(i & 1) * S1P_PLANE + q * 4] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid == 0) L.list_n = 0;
        if (tid < 12) L.nzrow[tid] = 0u;
        L.rows[rbuf ^ 1][row_slot] = (unsigned short)row_next;  // the next patch's rows (fetched during conv2)
        rbuf ^= 1;
        caelo_lds_barrier();
        j = jn;
        row = row_next;
        patch = patch_next;
        ENC_STAMP(5);
    }
#ifdef CAELO_ENC_PROF
    if (threadIdx.x == 0)
        for (int i = 0; i < 8; ++i) atomicAdd(&g_enc_stamp[i], (unsigned long long)L.prof[i]);
#endif
}
#define ENC_STAGE1_ARGS const caelo_enc_in in, int64_t n_patches, int group, int *__restrict__ work_counter,                      \
                        const float *__restrict__ w1g, const float *__restrict__ b1g, const float *__restrict__ w2g,              \
                        const float *__restrict__ c0g, float *__restrict__ p2out
__global__ void __launch_bounds__(256, 3) k_enc_stage1(ENC_STAGE1_ARGS) {
    enc_stage1_body<CAELO_ACT_TANH>(in, n_patches, group, work_counter, w1g, b1g, w2g, c0g, p2out);
}
__global__ void __launch_bounds__(256, 3) k_enc_stage1_relu(ENC_STAGE1_ARGS) {
    enc_stage1_body<CAELO_ACT_RELU>(in, n_patches, group, work_counter, w1g, b1g, w2g, c0g, p2out);
}
