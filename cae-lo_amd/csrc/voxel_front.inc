// voxel_front.inc -- the voxel tables' device helpers and the bodies of the one-pass build's kernels.
//
// One definition per body: voxel.hip's stand-alone kernels (k_vox_points, k_vox_coarse, k_vox_coarse2, k_vox_suspects_resolve) and
// ring.hip's fused front kernels, which run a body of the build in further workgroups of a key point launch, call the same
// function.  A body is told which workgroup of its role it is (and how many there are where it strides over them) instead of
// reading blockIdx itself; everything else is as it was inside the kernel.  __forceinline__ is part of the contract (DESIGN.md 6).
#pragma once

#define VOX_SIZE 0.02
#define BLOCK_REAL 1.28
#define VIS_L 99.84
#define VIS_W 99.84
#define VIS_H 14.72

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
// find-or-insert a key; returns slot or -1 when the table is full
__device__ inline int table_insert(unsigned long long *keys, uint32_t mask, unsigned long long key) {
    uint32_t h = caelo_hash64(key) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        unsigned long long k = keys[h];
        if (k == key) return (int)h;
        if (k == CAELO_EMPTY_KEY) {
            k = atomicCAS(&keys[h], CAELO_EMPTY_KEY, key);
            if (k == CAELO_EMPTY_KEY || k == key) return (int)h;
        }
        h = (h + 1) & mask;
    }
    return -1;
}

__device__ inline int table_find(const unsigned long long *keys, uint32_t mask, unsigned long long key) {
    uint32_t h = caelo_hash64(key) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long k = keys[h];
        if (k == key) return (int)h;
        if (k == CAELO_EMPTY_KEY) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// set the voxel's bit in its brick; returns 1 if the bit was newly set, 0 if present, -1 if full
__device__ inline int brick_set(caelo_brick_table t, int x, int y, int z) {
    const int slot = table_insert(t.keys, t.mask, caelo_pack3(x >> 3, y >> 3, z >> 3));
    if (slot < 0) return -1;
    const unsigned long long bit = 1ull << (((y & 7) << 3) | (z & 7));
    unsigned long long *w = &t.bits[(size_t)slot * 8 + (x & 7)];
    // Thousands of near-range points share one coarse voxel: test before the atomic so the word is
    // not hammered by read-modify-writes that change nothing (a stale 0 only costs one extra atomic).
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return 0;
    const unsigned long long old = atomicOr(w, bit);
    return (old & bit) ? 0 : 1;
}

// find-or-insert that also reports whether THIS call created the entry
__device__ inline int table_insert_new(unsigned long long *keys, uint32_t mask, unsigned long long key, bool *is_new) {
    uint32_t h = caelo_hash64(key) & mask;
    *is_new = false;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        unsigned long long k = keys[h];
        if (k == key) return (int)h;
        if (k == CAELO_EMPTY_KEY) {
            k = atomicCAS(&keys[h], CAELO_EMPTY_KEY, key);
            if (k == CAELO_EMPTY_KEY) { *is_new = true; return (int)h; }
            if (k == key) return (int)h;
        }
        h = (h + 1) & mask;
    }
    return -1;
}

// brick_mark that reports a newly created brick (the caller appends its slot to a compact list, one
// global atomic per workgroup, so the next pass runs on dense wavefronts)
__device__ inline bool brick_mark_new(caelo_brick_table t, int x, int y, int z, int *slot_out, bool *is_new) {
    const int slot = table_insert_new(t.keys, t.mask, caelo_pack3(x >> 3, y >> 3, z >> 3), is_new);
    *slot_out = slot;
    if (slot < 0) return false;
    const unsigned long long bit = 1ull << (((y & 7) << 3) | (z & 7));
    unsigned long long *w = &t.bits[(size_t)slot * 8 + (x & 7)];
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
        (void)__hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// fire-and-forget variant: no returned value -> a non-returning L2 atomic, no round trip.
// returns false only when the table is full.
__device__ inline bool brick_mark(caelo_brick_table t, int x, int y, int z) {
    const int slot = table_insert(t.keys, t.mask, caelo_pack3(x >> 3, y >> 3, z >> 3));
    if (slot < 0) return false;
    const unsigned long long bit = 1ull << (((y & 7) << 3) | (z & 7));
    unsigned long long *w = &t.bits[(size_t)slot * 8 + (x & 7)];
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
        (void)__hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

struct VoxIdx {
    int g[3];   // scale-0 global voxel index
    int v1[3];  // scale-1
    int v2[3];  // scale-2
    bool ok, oob, nonfinite;
};

// int(p / d) exactly as the reference's float64 division + truncation toward zero gives it (NumPy's int32 cast, Voxel.py:185,:193;
// |quotient| < 2^24, either sign: a given key point may lie off the voxel grid, CAELO_GIVEN_KEYPTS_RANGE), without the division for
// all but a few points: t = p * (1 / d) is within 2^24 x 5e-16 < 1e-8 of the true quotient, and so is the correctly rounded p / d, so
// whenever t sits further than 1e-6 from an integer both truncate alike; only a point within a micro-voxel of a voxel face (the
// points that make a metrically quantised scan interesting, 14 of 126 k) pays for v_div_f64's ~40 instructions.
__device__ inline int vox_trunc_div(double p, double d, double inv_d) {
    const double t = p * inv_d;
    const int n = (int)t;
    const double frac = fabs(t - (double)n);   // (t - n lies in (-1, 0] for t < 0)
    if (frac > 1e-6 && frac < 1.0 - 1e-6) return n;
    return (int)(p / d);
}

// Voxel.py:89-97,:118-152 for one point; f64 index math (SURVEY 8a-4)
__device__ inline VoxIdx voxel_indices(float fx, float fy, float fz) {
    VoxIdx r;
    r.ok = false;
    r.oob = false;
    r.nonfinite = fx != fx || fy != fy || fz != fz;   // NaN passes the filter below (abs(nan) > L is False) and int(nan) raises: Voxel.py:122
    if (r.nonfinite) return r;
    if (fabsf(fx) > (float)VIS_L || fabsf(fy) > (float)VIS_W || fabsf(fz) > (float)VIS_H) return r;  // :89-97
    const double p[3] = {(double)fx + VIS_L, (double)fy + VIS_W, (double)fz + VIS_H};                 // :118-120
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = vox_trunc_div(p[a], BLOCK_REAL, 1.0 / BLOCK_REAL);                        // :122-124
        const double rem = p[a] - b * BLOCK_REAL;                                               // :136-138 (may be -ulp: the division below)
        const int v = rem >= 0.0 ? vox_trunc_div(rem, VOX_SIZE, 1.0 / VOX_SIZE) : (int)(rem / VOX_SIZE);
        if (v < 0 || v >= 64) r.oob = true;
        r.g[a] = v + b * 64;                                                                    // :143
        r.v1[a] = vox_trunc_div(p[a], VOX_SIZE * 8, 1.0 / (VOX_SIZE * 8));                      // :147-149
        r.v2[a] = vox_trunc_div(p[a], VOX_SIZE * 32, 1.0 / (VOX_SIZE * 32));                    // :150-152
    }
    r.ok = !r.oob;
    return r;
}

// ------------------------------------------------------------------------------------------------
// K5 fast path (fused extract): one pass over the points + one pass over the scale-0 bricks.
// A scale-0 brick (8 x 0.02 m) IS a scale-1 voxel (0.16 m) and 4 of those a scale-2 voxel
// (Voxel.py:15-31), so scales 1/2 follow from the set of scale-0 bricks -- for every scale-0 voxel whose
// FIRST point (the only one that reaches layers 1/2, Voxel.py:139-158) has its own int(x_/0.16), int(x_/0.64)
// (Voxel.py:147-152) equal to its scale-0 index >> 3, >> 5.  A point with x_ within an ulp of a voxel face
// breaks that (x = 4.0 exactly; a few of every metrically quantised scan: 14 of 126 k points at mm resolution).
// Such points are handled exactly, without leaving the one-pass scheme:
//   * k_vox_points enters the voxel of every inconsistent point into a small "suspect" table (and counts the
//     suspect voxels of each brick);
//   * k_vox_coarse derives a scale-1 voxel from a brick only if the brick holds a NON-suspect voxel (all points of
//     such a voxel are consistent, so its first one is), k_vox_coarse2 derives scale 2 from those;
//   * k_vox_suspects_first / _resolve (empty launches when the frame has no inconsistent point) find the first point
//     of every suspect voxel (atomicMin over all points) and insert that point's own scale-1 / 2 indices -- exactly
//     what the reference's loop does when it meets the voxel for the first time.
// ------------------------------------------------------------------------------------------------
// Every kernel of the fast path is a body (one definition) behind a stand-alone kernel (voxel.hip) and, for the front chain that has
// no voxel stream, behind a fused kernel (ring.hip): the body is told which workgroup of its role it is, and how many there are
// where it strides over them.
static __device__ __forceinline__ void vox_points_body(const caelo_frame_dev &F, const unsigned int block) {
    const float *__restrict__ pc = F.pc;
    const int64_t n = F.n;
    const int stride = F.pc_stride;
    const caelo_brick_table b0 = F.brick[0];
    uint32_t *list0 = F.list0;
    int32_t *counts = F.counts, *status = F.status;
    const SuspectTables sp = F.sp;
    const int64_t i = (int64_t)block * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    VoxIdx v;
    v.ok = false;
    v.oob = false;
    v.nonfinite = false;
    if (i < n) {
        const float *p = pc + i * stride;
        v = voxel_indices(p[0], p[1], p[2]);
    }
    int st = (v.oob ? CAELO_ST_VOXEL_OOB : 0) | (v.nonfinite ? CAELO_ST_NONFINITE : 0);
    unsigned long long key = CAELO_EMPTY_KEY;
    // every point's scale-0 voxel, for k_vox_suspects_first (the fused build leaves the exact build's first-touch key table
    // free; it holds >= 1.5 entries per point, checked against the point count by the caller: indexed by the point here)
    if (i < n) F.vkeys[0][i] = v.ok ? caelo_pack3(v.g[0], v.g[1], v.g[2]) : CAELO_EMPTY_KEY;
    if (v.ok) {
        bool consistent = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) consistent &= (v.v1[a] == (v.g[a] >> 3)) && (v.v2[a] == (v.g[a] >> 5));
        key = caelo_pack3(v.g[0] >> 3, v.g[1] >> 3, v.g[2] >> 3);
        if (!consistent) {  // rare: its voxel becomes a suspect (tables hold >= 1.5 slots per point and at most one entry per point: load <= 0.67, never full)
            bool sp_new = false;
            const int ss = table_insert_new(sp.sp_keys, sp.mask, caelo_pack3(v.g[0], v.g[1], v.g[2]), &sp_new);
            uint32_t sb = 0xFFFFFFFFu;
            if (sp_new) {
                sb = (uint32_t)table_insert(sp.sb_keys, sp.mask, key);
                atomicAdd(&sp.sb_cnt[sb], 1u);  // 0xFFFFFFFF + 1 = 0: the entry holds (suspect voxels of the brick) - 1
            }
            sp.list[atomicAdd(&counts[6], 1)] = make_uint4((uint32_t)i, (uint32_t)ss, sb, 0u);
        }
    }
    // Neighbouring points of a scan line fall into the same 16 cm brick: only the first lane of each run of
    // equal keys walks the hash table (memory-side atomics cost microseconds), the run reuses its slot.
    // The chain of dependent memory round trips is what this kernel costs (86 % of its wave cycles wait), so it is kept to two:
    // the scan's point, then ONE compare-and-swap on the key's home slot (no look first: most heads create their brick) with the
    // workgroup's list reservation in flight beside it -- a slot for every head, reserved before anyone knows which heads are
    // new (the others leave holes, 0xFFFFFFFF, which the two readers of the list skip); the bit goes out as an atomic OR
    // nobody waits for.  (Round 2: load key -> CAS -> reserve -> load word -> OR, 44 us per 8 frames.)
    const unsigned long long prev = __shfl_up(key, 1);
    const bool head = v.ok && (lane == 0 || prev != key);
    const uint32_t h0 = caelo_hash64(key) & b0.mask;
    unsigned long long old = CAELO_EMPTY_KEY;
    if (head) old = atomicCAS(&b0.keys[h0], CAELO_EMPTY_KEY, key);
    __shared__ int s_tmp[2];
    const int lpos = caelo_block_reserve_async(&counts[4], head, s_tmp);  // ONE global atomic per workgroup
    int slot = -1;
    if (head) {
        bool is_new = old == CAELO_EMPTY_KEY;
        slot = (int)h0;
        if (!is_new && old != key) slot = table_insert_new(b0.keys, b0.mask, key, &is_new);  // home slot taken: probe on
        if (slot < 0) st |= CAELO_ST_MAP_FULL;
        list0[lpos] = is_new ? (uint32_t)slot : 0xFFFFFFFFu;
    }
    // The bits.  A memory-side atomic moves a 64-byte line there and back whatever it changes (one OR per point: 76 MB of
    // traffic for 16 MB of points, and the kernel's time): the wave first ORs its points into an LDS image of the bricks it
    // touches -- row = run of equal keys, 8 words each -- and then issues one atomic per non-empty word.
    __shared__ unsigned long long s_agg[4][64][8];
    __shared__ int s_slot[4][64];
    const int wave = threadIdx.x >> 6;
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = heads & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));  // heads at or below this lane
    const int run = __popcll(upto) - 1;                                                        // (-1: no head yet -> not ok either)
    const int nruns = __popcll(heads);
#pragma unroll
    for (int w = 0; w < 8; w += 2) *(ulonglong2 *)&s_agg[wave][lane][w] = make_ulonglong2(0ull, 0ull);
    if (head) s_slot[wave][run] = slot;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (v.ok) atomicOr(&s_agg[wave][run][v.g[0] & 7], 1ull << (((v.g[1] & 7) << 3) | (v.g[2] & 7)));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {   // lane (r, w) = (lane >> 3, lane & 7) flushes word w of runs r, r + 8, ...
        const int w = lane & 7;
        for (int r = lane >> 3; r < nruns; r += 8) {
            const unsigned long long bitsw = s_agg[wave][r][w];
            const int sl = s_slot[wave][r];
            if (bitsw && sl >= 0)
                (void)__hip_atomic_fetch_or(&b0.bits[(size_t)sl * 8 + w], bitsw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (st) atomicOr(status, st);
}

// The suspect voxels of the frame (see the header of this section) take two steps that have nothing to do -- one word read
// per workgroup -- when no point of the frame was inconsistent.  (A single kernel whose last workgroup resolves would need an
// agent-scope release per workgroup: on gfx950 that is an L2 write-back walk, 433 us for 8 frames.)
// (1) first point of every suspect voxel: smallest index over ALL points of the voxel, consistent ones included.  Runs in extra
//     workgroups of k_vox_coarse's launch (both only need k_vox_points done; both are chains of dependent memory round trips
//     that leave the CUs idle: side by side they cost the longer of the two, 32 us, instead of 32 + 14)
#define SUSPECT_LDS 128
static __device__ __forceinline__ void vox_suspects_first(const caelo_frame_dev &F, int block) {
    const int nsp = F.counts[6];
    if (nsp == 0) return;
    // A handful of voxels (14 of a 126 k-point scan quantised to 1 mm): the workgroup stages their keys in LDS and every point
    // compares the key k_vox_points stored for it against them -- no index arithmetic, no table probe per point (both together
    // were 15.7 us per 8 frames for those 14 voxels).  More inconsistent points than the LDS list holds: probe the table.
    __shared__ unsigned long long s_key[SUSPECT_LDS];
    __shared__ uint32_t s_slot[SUSPECT_LDS];
    const bool listed = nsp <= SUSPECT_LDS;
    if (listed) {
        if ((int)threadIdx.x < nsp) {
            const uint32_t ss = F.sp.list[threadIdx.x].y;
            s_slot[threadIdx.x] = ss;
            s_key[threadIdx.x] = F.sp.sp_keys[ss];
        }
        __syncthreads();
    }
    const int64_t i = (int64_t)block * blockDim.x + threadIdx.x;
    if (i >= F.n) return;
    const unsigned long long key = F.vkeys[0][i];
    if (key == CAELO_EMPTY_KEY) return;
    if (listed) {
        for (int e = 0; e < nsp; ++e)  // (several inconsistent points of one voxel repeat its key: the same atomicMin twice)
            if (s_key[e] == key) { atomicMin(&F.sp.sp_first[s_slot[e]], (uint32_t)i); break; }
    } else {
        const int ss = table_find(F.sp.sp_keys, F.sp.mask, key);
        if (ss >= 0) atomicMin(&F.sp.sp_first[ss], (uint32_t)i);
    }
}

// the occupied scale-0 bricks (256 per workgroup iteration): a brick is a scale-1 voxel, and counts its voxels
#define COARSE_WGS 256
// block: below COARSE_WGS a workgroup of the brick pass, from there on one of vox_suspects_first
static __device__ __forceinline__ void vox_coarse_body(const caelo_frame_dev &F, const unsigned int block) {
    if (block >= COARSE_WGS) {  // (workgroup-uniform)
        vox_suspects_first(F, (int)block - COARSE_WGS);
        return;
    }
    const caelo_brick_table b0 = F.brick[0], b1 = F.brick[1];
    const uint32_t *list0 = F.list0;
    uint32_t *list1 = F.list1;
    int32_t *counts = F.counts, *status = F.status;
    const SuspectTables sp = F.sp;
    __shared__ int s_tmp[2];
    const int nb = counts[4];
    const bool any_suspect = counts[6] > 0;
    int pop = 0;
    for (int i0 = block * blockDim.x; i0 < nb; i0 += COARSE_WGS * blockDim.x) {  // uniform trip count per workgroup
        const int i = i0 + threadIdx.x;
        bool is_new = false;
        int slot1 = -1;
        const uint32_t slot = i < nb ? list0[i] : 0xFFFFFFFFu;
        if (slot != 0xFFFFFFFFu) {  // (list0 has holes, see k_vox_points)
            const unsigned long long k = b0.keys[slot];
            const ulonglong2 *w = (const ulonglong2 *)(b0.bits + (size_t)slot * 8);
            int mine = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { const ulonglong2 u = w[q]; mine += __popcll(u.x) + __popcll(u.y); }
            pop += mine;
            if (any_suspect) {  // voxels whose first point may disagree with the brick are left to k_vox_suspects
                const int sb = table_find(sp.sb_keys, sp.mask, k);
                if (sb >= 0) mine -= (int)(sp.sb_cnt[sb] + 1u);
            }
            const int x = (int)((k >> 40) & 0xFFFFF), y = (int)((k >> 20) & 0xFFFFF), z = (int)(k & 0xFFFFF);
            if (mine > 0 && !brick_mark_new(b1, x, y, z, &slot1, &is_new)) atomicOr(status, CAELO_ST_MAP_FULL);
        }
        const int lpos = caelo_block_reserve(&counts[5], is_new, s_tmp);
        if (is_new) list1[lpos] = (uint32_t)slot1;
    }
    caelo_block_add(&counts[0], pop, s_tmp);
}

// the occupied scale-1 bricks: count their voxels and mark the scale-2 voxels under them
// (a scale-1 brick spans 2x2x2 scale-2 voxels: scale-2 index = scale-1 index >> 2)
static __device__ __forceinline__ void vox_coarse2_body(const caelo_frame_dev &F, const unsigned int block, const unsigned int nblocks) {
    const caelo_brick_table b1 = F.brick[1], b2 = F.brick[2];
    const uint32_t *list1 = F.list1;
    int32_t *counts = F.counts, *status = F.status;
    __shared__ int s_tmp[2];
    const int nb = counts[5];
    int pop = 0, pop2 = 0;
    for (int i = block * blockDim.x + threadIdx.x; i < nb; i += nblocks * blockDim.x) {
        const uint32_t slot = list1[i];
        const unsigned long long k = b1.keys[slot];
        const int bx = (int)((k >> 40) & 0xFFFFF) << 3, by = (int)((k >> 20) & 0xFFFFF) << 3, bz = (int)(k & 0xFFFFF) << 3;
        const unsigned long long *w = b1.bits + (size_t)slot * 8;
        // The 2x2x2 scale-2 voxels under this brick all live in ONE scale-2 brick (index >> 2): one table
        // insert, then one OR per x-half with the (hy, hz) bits gathered -- not eight insert+OR chains of
        // memory-side atomics.  Octant (hx, hy, hz): words x in [4hx, 4hx+4), bits y in [4hy, ..), z in [4hz, ..)
        unsigned long long orv[2] = {0ull, 0ull};
#pragma unroll
        for (int hx = 0; hx < 2; ++hx) {
            const unsigned long long m = w[4 * hx] | w[4 * hx + 1] | w[4 * hx + 2] | w[4 * hx + 3];
            pop += __popcll(w[4 * hx]) + __popcll(w[4 * hx + 1]) + __popcll(w[4 * hx + 2]) + __popcll(w[4 * hx + 3]);
#pragma unroll
            for (int hy = 0; hy < 2; ++hy)
#pragma unroll
                for (int hz = 0; hz < 2; ++hz) {
                    const unsigned long long sel = (0x0F0F0F0Full << (4 * hz)) << (32 * hy);
                    const int y2 = (by >> 2) + hy, z2 = (bz >> 2) + hz;
                    if (m & sel) orv[hx] |= 1ull << (((y2 & 7) << 3) | (z2 & 7));
                }
        }
        if (orv[0] | orv[1]) {
            const int x2 = bx >> 2;  // even: x2 and x2 + 1 share the scale-2 brick
            const int slot2 = table_insert(b2.keys, b2.mask, caelo_pack3(x2 >> 3, by >> 5, bz >> 5));
            if (slot2 < 0) atomicOr(status, CAELO_ST_MAP_FULL);
            else {
#pragma unroll
                for (int hx = 0; hx < 2; ++hx) {
                    if (!orv[hx]) continue;
                    unsigned long long *wd = &b2.bits[(size_t)slot2 * 8 + ((x2 + hx) & 7)];
                    if ((__hip_atomic_load(wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & orv[hx]) != orv[hx]) {
                        // every scale-2 voxel is counted by the one atomic that sets its bit (no separate counting pass)
                        const unsigned long long old = __hip_atomic_fetch_or(wd, orv[hx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pop2 += __popcll(orv[hx] & ~old);
                    }
                }
            }
        }
    }
    caelo_block_add(&counts[1], pop, s_tmp);
    __syncthreads();  // s_tmp is reused
    caelo_block_add(&counts[2], pop2, s_tmp);
}

#define COARSE2_WGS 64

// (2) that point's own scale-1 / 2 indices are inserted, exactly what the reference's loop does when it meets the voxel
// (its stride loop makes the workgroup's size irrelevant: 256 threads stand-alone, 1024 beside k_kp_hist)
static __device__ __forceinline__ void vox_suspects_resolve_body(const caelo_frame_dev &F, const unsigned int block, const unsigned int nblocks) {
    const float *__restrict__ pc = F.pc;
    const int stride = F.pc_stride;
    const caelo_brick_table b1 = F.brick[1], b2 = F.brick[2];
    uint32_t *list1 = F.list1;
    int32_t *counts = F.counts, *status = F.status;
    const SuspectTables sp = F.sp;
    const int nsp = counts[6];
    for (int e = block * blockDim.x + threadIdx.x; e < nsp; e += nblocks * blockDim.x) {
        const uint4 ent = sp.list[e];
        const uint32_t j = sp.sp_first[ent.y];
        const float *p = pc + (int64_t)j * stride;
        const VoxIdx v = voxel_indices(p[0], p[1], p[2]);  // the voxel's first point: its own scale-1 / 2 indices count
        // several inconsistent points of one voxel repeat this: idempotent, the counters only see bits that were new
        bool is_new = false;
        const int s1 = table_insert_new(b1.keys, b1.mask, caelo_pack3(v.v1[0] >> 3, v.v1[1] >> 3, v.v1[2] >> 3), &is_new);
        if (s1 < 0) atomicOr(status, CAELO_ST_MAP_FULL);
        else {
            if (is_new) list1[atomicAdd(&counts[5], 1)] = (uint32_t)s1;
            const unsigned long long bit = 1ull << (((v.v1[1] & 7) << 3) | (v.v1[2] & 7));
            if (!(atomicOr(&b1.bits[(size_t)s1 * 8 + (v.v1[0] & 7)], bit) & bit)) atomicAdd(&counts[1], 1);
        }
        const int r2 = brick_set(b2, v.v2[0], v.v2[1], v.v2[2]);
        if (r2 < 0) atomicOr(status, CAELO_ST_MAP_FULL);
        else if (r2) atomicAdd(&counts[2], 1);
    }
}
