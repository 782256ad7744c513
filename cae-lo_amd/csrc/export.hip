// export.hip -- AllVoxels0/1/2 in the reference's exact order (off the hot path; API parity for
// Voxelization(PC), Voxel.py:100-173).
//
// The reference appends a voxel the first time a point touches it: AllVoxels1/2 are in first-touch
// order (Voxel.py:153-158); AllVoxels0 is grouped by 64^3 block, blocks in first-touch order, voxels
// in first-touch order inside a block (Voxel.py:126-143,:161-165).  The voxel map already records
// the smallest point index touching every voxel, so the order is a sort by that index -- by
// (first index of the block, first index of the voxel) for scale 0.  The sort itself is rocPRIM's
// device radix sort (a library primitive, like a memcpy; none of the hot-path kernels use a library).
#include <cstring>

#include "caelo_internal.h"

#include <rocprim/rocprim.hpp>

// forward: helpers shared with voxel.hip are small enough to restate
__device__ static inline int exp_table_insert(unsigned long long *keys, uint32_t mask, unsigned long long key) {
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

__device__ static inline unsigned long long block_of(unsigned long long vkey) {
    const unsigned x = (unsigned)(vkey >> 40) & 0xFFFFF, y = (unsigned)(vkey >> 20) & 0xFFFFF, z = (unsigned)vkey & 0xFFFFF;
    return caelo_pack3((int)(x >> 6), (int)(y >> 6), (int)(z >> 6));
}

__global__ void __launch_bounds__(256) k_exp_block_first(const unsigned long long *__restrict__ vkeys,
                                                         const uint32_t *__restrict__ vfirst, uint32_t vmask,
                                                         unsigned long long *bkeys, uint32_t *bfirst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > vmask) return;
    const unsigned long long k = vkeys[i];
    if (k == CAELO_EMPTY_KEY) return;
    const int s = exp_table_insert(bkeys, vmask, block_of(k));
    if (s >= 0) atomicMin(&bfirst[s], vfirst[i]);
}

__global__ void __launch_bounds__(256) k_exp_compact(const unsigned long long *__restrict__ vkeys,
                                                     const uint32_t *__restrict__ vfirst, uint32_t vmask,
                                                     const unsigned long long *__restrict__ bkeys,
                                                     const uint32_t *__restrict__ bfirst, int use_block,
                                                     unsigned long long *skeys, unsigned long long *svals, int32_t *count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > vmask) return;
    const unsigned long long k = vkeys[i];
    if (k == CAELO_EMPTY_KEY) return;
    unsigned long long sk = (unsigned long long)(unsigned)vfirst[i];
    if (use_block) {
        const unsigned long long bk = block_of(k);
        uint32_t h = caelo_hash64(bk) & vmask;
        while (bkeys[h] != bk) h = (h + 1) & vmask;
        sk |= (unsigned long long)(unsigned)bfirst[h] << 32;
    }
    const int p = atomicAdd(count, 1);
    skeys[p] = sk;
    svals[p] = k;
}

// the sorted run is `*count` long (a device word: the call never waits for it); the rest of the padded sort is 0xFF.. keys
__global__ void __launch_bounds__(256) k_exp_write(const unsigned long long *__restrict__ svals, const int32_t *__restrict__ count,
                                                   int64_t capacity, int16_t *__restrict__ out, int64_t *__restrict__ count_out64,
                                                   int32_t *__restrict__ count_out32) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *count;
    if (i == 0) {
        if (count_out64) *count_out64 = n;
        if (count_out32) *count_out32 = n;
    }
    if (i >= n || i >= capacity) return;
    const unsigned long long k = svals[i];
    out[3 * i] = (int16_t)((k >> 40) & 0xFFFFF);
    out[3 * i + 1] = (int16_t)((k >> 20) & 0xFFFFF);
    out[3 * i + 2] = (int16_t)(k & 0xFFFFF);
}

// The lists of the scales in `mask`, each in first-touch order, written to outs[scale] (device), their lengths to counts64[scale] /
// counts32[scale] (device; either may be null).  No host round trip: every scale is sorted at its table's size with 0xFF.. keys
// behind the `count` real ones (a few hundred microseconds of sorting more than the exact length would take, against four stream
// synchronisations per call -- which is what serialised the tie redo of many frames on side streams, Engine.resolve_ties_many).
static int export_scales(caelo_voxmap *m, int mask, int16_t *const outs[3], int64_t capacity, int64_t *counts64, int32_t *counts32, hipStream_t s) {
    const size_t vs = (size_t)m->vmask[0] + 1;
    // scratch: block table (keys + first) | sort keys in/out | sort vals in/out | count | rocprim temp
    size_t temp_bytes = 0;
    CAELO_HIP(rocprim::radix_sort_pairs((void *)nullptr, temp_bytes, (unsigned long long *)nullptr,
                                        (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                        (unsigned long long *)nullptr, vs, 0, 64, s));
    const size_t need = vs * (8 + 4) + 4 * vs * 8 + 64 + temp_bytes;
    if ((size_t)m->scratch_bytes < need) {
        if (m->scratch) CAELO_HIP(hipFree(m->scratch));
        CAELO_HIP(hipMalloc(&m->scratch, need));
        m->scratch_bytes = (int64_t)need;
    }
    char *base = (char *)m->scratch;
    unsigned long long *bkeys = (unsigned long long *)base;
    unsigned long long *k_in = bkeys + vs, *k_out = k_in + vs, *v_in = k_out + vs, *v_out = v_in + vs;
    uint32_t *bfirst = (uint32_t *)(v_out + vs);
    int32_t *count = (int32_t *)(bfirst + vs);
    void *temp = (void *)(count + 16);
    for (int sc = 0; sc < 3; ++sc) {
        if (!(mask >> sc & 1)) continue;
        const size_t vsc = (size_t)m->vmask[sc] + 1;
        const unsigned grid = (unsigned)((vsc + 255) / 256);
        CAELO_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), s));
        if (sc == 0) {
            CAELO_HIP(hipMemsetAsync(bkeys, 0xFF, vs * 8, s));
            CAELO_HIP(hipMemsetAsync(bfirst, 0xFF, vs * 4, s));
            k_exp_block_first<<<grid, 256, 0, s>>>(m->vkeys[0], m->vfirst[0], m->vmask[0], bkeys, bfirst);
            CAELO_LAUNCH_CHECK();
        }
        CAELO_HIP(hipMemsetAsync(k_in, 0xFF, vsc * 8, s));
        k_exp_compact<<<grid, 256, 0, s>>>(m->vkeys[sc], m->vfirst[sc], m->vmask[sc], bkeys, bfirst, sc == 0, k_in, v_in, count);
        CAELO_LAUNCH_CHECK();
        size_t tb = temp_bytes;
        CAELO_HIP(rocprim::radix_sort_pairs(temp, tb, k_in, k_out, v_in, v_out, vsc, 0, 64, s));
        k_exp_write<<<grid, 256, 0, s>>>(v_out, count, capacity, outs[sc], counts64 ? counts64 + sc : nullptr, counts32 ? counts32 + sc : nullptr);
        CAELO_LAUNCH_CHECK();
    }
    return CAELO_OK;
}

CAELO_API int caelo_voxmap_export(caelo_ctx *c, caelo_voxmap *m, int16_t *all0, int16_t *all1, int16_t *all2,
                                  int64_t capacity, int64_t *counts, void *stream) {
    CAELO_REQUIRE(c && m && all0 && all1 && all2 && counts, "null argument");
    CAELO_REQUIRE(m->order_tracked, "caelo_voxmap_export: the map was not filled by caelo_voxelize (no first-touch order)");
    int16_t *const outs[3] = {all0, all1, all2};
    return export_scales(m, 7, outs, capacity, counts, nullptr, caelo_stream(stream));
}

CAELO_API int caelo_voxmap_order(caelo_ctx *c, caelo_voxmap *m, int scale_mask, void *stream) {
    CAELO_REQUIRE(c && m, "null argument");
    CAELO_REQUIRE(m->order_tracked, "caelo_voxmap_order: the map was not filled by caelo_voxelize (no first-touch order)");
    hipStream_t s = caelo_stream(stream);
    int16_t *outs[3];
    int32_t *n_out = nullptr;
    const int rc = kd_begin_device_lists(m, outs, &n_out, s);
    if (rc != CAELO_OK) return rc;
    return export_scales(m, scale_mask & 7, outs, m->max_points, nullptr, n_out, s);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// CAELO_EXTRACT_EXACT_PATCHES: the same lists for a frame SET inside the fused path, with the host never reading anything.
// After k_patches, k_xo_census counts each frame's tie-split patches (flags & 2) per scale into its kd state words; every later kernel
// reads that count and leaves at once for a (frame, scale) with nothing tied, whose list length stays 0 -- so the kd kernels behind
// them (kdorder.hip) find empty queues there.  The lists of the tied pairs are sorted by ONE segmented radix sort over the set: segment
// (frame, scale) = [seg * cap, end[seg]) of the set leader's buffers, end[] grown on the device by the compaction (an empty segment
// costs the sort nothing).  A sort key is (first point of the voxel's 64^3 block << B) | first point of the voxel for scale 0 and the
// voxel's first point for scales 1 / 2 (B bits hold any point index of the map); the value is the voxel's slot in its first-touch
// table.  Keys are distinct (a point opens one voxel per scale), so the order is the reference's.
// ------------------------------------------------------------------------------------------------------------------------------------
namespace {

struct XoLayout {
    size_t bkeys, bfirst, keys0, keys1, vals0, vals1, begin, end, temp, temp_bytes, total;
    int64_t cap;
    int kbits;
};

size_t xo_align(size_t v) { return (v + 255) & ~(size_t)255; }

// nf = frames of the sets this map leads (0: it only ever is a later frame of a set -- block table only)
int xo_layout(const caelo_voxmap *m, int nf, XoLayout &L) {
    const size_t vs = (size_t)m->vmask[0] + 1;
    L.cap = m->max_points;
    L.kbits = 1;
    while (((int64_t)1 << L.kbits) < L.cap) ++L.kbits;
    size_t off = 0;
    L.bkeys = off; off += xo_align(vs * 8);
    L.bfirst = off; off += xo_align(vs * 4);
    L.keys0 = L.keys1 = L.vals0 = L.vals1 = L.begin = L.end = L.temp = off;
    L.temp_bytes = 0;
    if (nf > 0) {
        const size_t el = (size_t)nf * 3 * (size_t)L.cap;
        L.keys0 = off; off += xo_align(el * 8);
        L.keys1 = off; off += xo_align(el * 8);
        L.vals0 = off; off += xo_align(el * 4);
        L.vals1 = off; off += xo_align(el * 4);
        L.begin = off; off += xo_align((size_t)nf * 3 * 4);
        L.end = off; off += xo_align((size_t)nf * 3 * 4);
        rocprim::double_buffer<unsigned long long> dk(nullptr, nullptr);
        rocprim::double_buffer<uint32_t> dv(nullptr, nullptr);
        CAELO_HIP(rocprim::segmented_radix_sort_pairs((void *)nullptr, L.temp_bytes, dk, dv, (unsigned)el, (unsigned)(nf * 3), (int32_t *)nullptr,
                                                      (int32_t *)nullptr, 0, 2 * L.kbits, (hipStream_t)0));
        L.temp = off; off += xo_align(L.temp_bytes);
    }
    L.total = off;
    return CAELO_OK;
}

struct XoFrame {
    const uint8_t *flags;
    const int32_t *n_key;
    int32_t *state;                        // the map's kd state words: [16 + sc] list lengths (out), [KD_ST_CENSUS + sc] census
    int16_t *vox[3];                       // the kd lists (out), vcap entries each
    int64_t vcap;
    const unsigned long long *vkeys[3];    // first-touch tables of the map
    const uint32_t *vfirst[3];
    unsigned long long *bkeys;             // block table of scale 0 (the map's ordering scratch)
    uint32_t *bfirst;
    uint32_t vmask;
};
struct XoSet {
    XoFrame f[CAELO_FB_MAX];
    unsigned long long *keys;   // the sort's input: [n * 3][cap]
    uint32_t *vals;
    int32_t *end;               // [n * 3] segment ends (begins: seg * cap)
    int64_t cap;
    int32_t kbits, n;
};
static_assert(sizeof(XoSet) <= 3800, "XoSet must fit the kernel argument segment");

constexpr unsigned XO_GRID = 1024;   // workgroups per (frame, scale) of the grid-stride kernels over a first-touch table

// one thread per (key point, scale) of frame blockIdx.z; also opens the frame's three segments
__global__ void __launch_bounds__(256) k_xo_census(const XoSet S) {
    const XoFrame &F = S.f[blockIdx.z];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        const int seg = blockIdx.z * 3 + threadIdx.x;
        S.end[seg] = (int32_t)(seg * S.cap);
    }
    if (t >= CAELO_FRAME_PATCHES) return;
    const int K = min(*F.n_key, CAELO_MAX_KEYPTS);
    if (t / 3 < K && (F.flags[t] & 2)) atomicAdd(&F.state[KD_ST_CENSUS + t % 3], 1);
}

__global__ void __launch_bounds__(256) k_xo_block_clear(const XoSet S) {
    const XoFrame &F = S.f[blockIdx.z];
    if (F.state[KD_ST_CENSUS] == 0) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= F.vmask; i += gridDim.x * blockDim.x) {
        F.bkeys[i] = CAELO_EMPTY_KEY;
        F.bfirst[i] = 0xFFFFFFFFu;
    }
}

__global__ void __launch_bounds__(256) k_xo_block_first(const XoSet S) {
    const XoFrame &F = S.f[blockIdx.z];
    if (F.state[KD_ST_CENSUS] == 0) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= F.vmask; i += gridDim.x * blockDim.x) {
        const unsigned long long k = F.vkeys[0][i];
        if (k == CAELO_EMPTY_KEY) continue;
        const int s = exp_table_insert(F.bkeys, F.vmask, block_of(k));
        if (s >= 0) atomicMin(&F.bfirst[s], F.vfirst[0][i]);
    }
}

// blockIdx.y = scale: the occupied slots of the first-touch table -> (key, slot) pairs at the end of the segment
__global__ void __launch_bounds__(256) k_xo_compact(const XoSet S) {
    const XoFrame &F = S.f[blockIdx.z];
    const int sc = blockIdx.y;
    if (F.state[KD_ST_CENSUS + sc] == 0) return;   // (uniform over the workgroup: before any barrier)
    __shared__ int s_tmp[2];
    const int seg = blockIdx.z * 3 + sc;
    const int64_t base = (int64_t)seg * S.cap;
    const unsigned long long *__restrict__ vkeys = F.vkeys[sc];
    const uint32_t *__restrict__ vfirst = F.vfirst[sc];
    for (uint32_t b0 = blockIdx.x * blockDim.x; b0 <= F.vmask; b0 += gridDim.x * blockDim.x) {   // (a uniform trip count)
        const uint32_t i = b0 + threadIdx.x;
        const unsigned long long k = i <= F.vmask ? vkeys[i] : CAELO_EMPTY_KEY;
        const bool occ = k != CAELO_EMPTY_KEY;
        unsigned long long key = 0;
        if (occ) {
            key = vfirst[i];
            if (sc == 0) {
                const unsigned long long bk = block_of(k);
                uint32_t h = caelo_hash64(bk) & F.vmask;
                for (uint32_t probe = 0; probe <= F.vmask && F.bkeys[h] != bk; ++probe) h = (h + 1) & F.vmask;
                key |= (unsigned long long)F.bfirst[h] << S.kbits;
            }
        }
        const int p = caelo_block_reserve(&S.end[seg], occ, s_tmp);
        if (occ && p - base < S.cap) {   // (always: a map holds at most max_points <= cap voxels per scale)
            S.keys[p] = key;
            S.vals[p] = i;
        }
    }
}

// the sorted segment -> the kd list of the map (scale blockIdx.y), its length -> the state word the kd kernels read
__global__ void __launch_bounds__(256) k_xo_write(const XoSet S, const uint32_t *__restrict__ vals) {
    const XoFrame &F = S.f[blockIdx.z];
    const int sc = blockIdx.y;
    const int seg = blockIdx.z * 3 + sc;
    const int64_t base = (int64_t)seg * S.cap;
    const int n = (int)min((int64_t)S.end[seg] - base, F.vcap);   // 0 for a (frame, scale) without a tie (never clipped: voxels <= points)
    if (blockIdx.x == 0 && threadIdx.x == 0) F.state[16 + sc] = n;
    const unsigned long long *__restrict__ vkeys = F.vkeys[sc];
    int16_t *__restrict__ out = F.vox[sc];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t slot = vals[base + i];
        const unsigned long long k = slot <= F.vmask ? vkeys[slot] : 0ull;
        out[3 * i] = (int16_t)((k >> 40) & 0xFFFFF);
        out[3 * i + 1] = (int16_t)((k >> 20) & 0xFFFFF);
        out[3 * i + 2] = (int16_t)(k & 0xFFFFF);
    }
}

}  // namespace

int exact_patches_prepare(caelo_voxmap *const *maps, int n_frames) {
    CAELO_REQUIRE(n_frames >= 1 && n_frames <= CAELO_FB_MAX, "exact_patches_prepare: 1 .. 8 frames");
    for (int i = 0; i < n_frames; ++i) {
        caelo_voxmap *m = maps[i];
        CAELO_REQUIRE(m->max_points <= maps[0]->max_points, "CAELO_EXTRACT_EXACT_PATCHES: frame 0's map must be the largest of a set");
        CAELO_REQUIRE(m->max_points * 3 * CAELO_FB_MAX < (int64_t)1 << 31, "CAELO_EXTRACT_EXACT_PATCHES: map too large for 32-bit sort offsets");
        int16_t *vox[3];
        int32_t *state;
        int rc = kd_fused_storage(m, vox, &state);
        if (rc != CAELO_OK) return rc;
        const int nf = i == 0 ? n_frames : 0;
        if (m->xo_base && m->xo_frames >= nf) continue;
        XoLayout L;
        if ((rc = xo_layout(m, nf, L))) return rc;
        if (m->xo_base) CAELO_HIP(hipFree(m->xo_base));
        m->xo_base = nullptr;
        m->xo_frames = 0;
        if (hipMalloc((void **)&m->xo_base, L.total) != hipSuccess) {
            m->xo_base = nullptr;
            caelo_set_error("CAELO_EXTRACT_EXACT_PATCHES: out of device memory (%zu bytes of ordering scratch)", L.total);
            return CAELO_ERR_HIP;
        }
        m->xo_bytes = L.total;
        if (nf > 0) {   // the segments' begins never change
            int32_t begin[CAELO_FB_MAX * 3];
            for (int s = 0; s < nf * 3; ++s) begin[s] = (int32_t)(s * L.cap);
            CAELO_HIP(hipMemcpy(m->xo_base + L.begin, begin, (size_t)nf * 3 * 4, hipMemcpyHostToDevice));
        }
        m->xo_frames = nf;
    }
    return CAELO_OK;
}

void exact_patches_clear_item(caelo_voxmap *m, caelo_clear_list &list) {
    int16_t *vox[3];
    int32_t *state = nullptr;
    if (kd_fused_storage(m, vox, &state) == CAELO_OK) list.item[list.n++] = {state, 256, 0u};   // (allocated by exact_patches_prepare)
}

int exact_patches_redo(caelo_voxmap *const *maps, const caelo_frame_set &fs, const caelo_extract_args *args, int n, hipStream_t s) {
    CAELO_REQUIRE(n >= 1 && n <= CAELO_FB_MAX, "exact_patches_redo: 1 .. 8 frames");
    caelo_voxmap *lead = maps[0];
    CAELO_REQUIRE(lead->xo_base && lead->xo_frames >= n, "internal: exact_patches_prepare was not called for this set");
    XoLayout L;
    int rc = xo_layout(lead, lead->xo_frames, L);   // (the scratch is laid out for the largest set: a partial set uses its first segments)
    if (rc) return rc;
    XoSet S = {};
    S.n = n;
    S.cap = L.cap;
    S.kbits = L.kbits;
    S.keys = (unsigned long long *)(lead->xo_base + L.keys0);
    S.vals = (uint32_t *)(lead->xo_base + L.vals0);
    S.end = (int32_t *)(lead->xo_base + L.end);
    const float *pts[CAELO_FB_MAX];
    const int32_t *nks[CAELO_FB_MAX];
    uint64_t *bits[CAELO_FB_MAX];
    uint8_t *flags[CAELO_FB_MAX];
    int32_t *status[CAELO_FB_MAX];
    for (int i = 0; i < n; ++i) {
        caelo_voxmap *m = maps[i];
        CAELO_REQUIRE(m->xo_base && m->order_tracked, "internal: a map of the set has no first-touch tables / ordering scratch");
        CAELO_REQUIRE(m->vmask[1] == m->vmask[0] && m->vmask[2] == m->vmask[0], "internal: first-touch tables of unequal sizes");
        CAELO_REQUIRE(args[i].kp_ld == args[0].kp_ld, "the frames of a set share the key points' leading dimension");
        XoFrame &F = S.f[i];
        if ((rc = kd_fused_storage(m, F.vox, &F.state))) return rc;
        F.flags = args[i].flags;
        F.n_key = args[i].n_key;
        for (int sc = 0; sc < 3; ++sc) { F.vkeys[sc] = m->vkeys[sc]; F.vfirst[sc] = m->vfirst[sc]; }
        F.bkeys = (unsigned long long *)m->xo_base;                        // (XoLayout: the block table leads every map's scratch)
        F.bfirst = (uint32_t *)(m->xo_base + xo_align(((size_t)m->vmask[0] + 1) * 8));
        F.vmask = m->vmask[0];
        F.vcap = m->max_points;   // (kd_alloc: the lists hold max_points entries)
        pts[i] = args[i].key_pts; nks[i] = args[i].n_key; bits[i] = (uint64_t *)fs.f[i].bits; flags[i] = args[i].flags; status[i] = args[i].status;
    }
    const size_t tblocks = ((size_t)lead->vmask[0] + 256) / 256;
    const unsigned tgrid = tblocks < XO_GRID ? (unsigned)tblocks : XO_GRID;
    k_xo_census<<<dim3((CAELO_FRAME_PATCHES + 255) / 256, 1, n), 256, 0, s>>>(S);
    CAELO_LAUNCH_CHECK();
    k_xo_block_clear<<<dim3(tgrid, 1, n), 256, 0, s>>>(S);
    CAELO_LAUNCH_CHECK();
    k_xo_block_first<<<dim3(tgrid, 1, n), 256, 0, s>>>(S);
    CAELO_LAUNCH_CHECK();
    k_xo_compact<<<dim3(tgrid, 3, n), 256, 0, s>>>(S);
    CAELO_LAUNCH_CHECK();
    rocprim::double_buffer<unsigned long long> dk(S.keys, (unsigned long long *)(lead->xo_base + L.keys1));
    rocprim::double_buffer<uint32_t> dv(S.vals, (uint32_t *)(lead->xo_base + L.vals1));
    size_t tb = L.temp_bytes;
    CAELO_HIP(rocprim::segmented_radix_sort_pairs((void *)(lead->xo_base + L.temp), tb, dk, dv, (unsigned)((size_t)n * 3 * L.cap), (unsigned)(n * 3),
                                                  (const int32_t *)(lead->xo_base + L.begin), (const int32_t *)S.end, 0, 2 * L.kbits, s));
    k_xo_write<<<dim3(256, 3, n), 256, 0, s>>>(S, dv.current());
    CAELO_LAUNCH_CHECK();
    for (int i = 0; i < n; ++i) maps[i]->kd_lists = true;   // (the lists of the untied scales are empty: their kd kernels leave at once)
    if ((rc = kd_resolve_many(n, maps, pts, args[0].kp_ld, CAELO_MAX_KEYPTS, nks, bits, flags, s, /*queues_clear*/ true))) return rc;
    return kd_report_left(n, maps, status, s);
}
