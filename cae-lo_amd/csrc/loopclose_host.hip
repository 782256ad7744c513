// loopclose_host.hip -- the host twins of the loop-closure kernels (loopclose.hip): host code only (no device call, no HIP header), so
// that it also links into a plain C++ program (tools/micro/loopclose_main.cpp runs it under the host sanitizers).  The same
// definitions (loopclose_common.h) with fmaf, sqrtf and / in the same order as the kernels.
#include "loopclose_common.h"

#define LC_API extern "C" __attribute__((visibility("default")))

LC_API int caelo_host_scan_context(const float *pts, int64_t ld, int cols, const int32_t *n_pts, int64_t n_frames, float *sc, float *u,
                                      uint64_t *valid) {
    SC_REQUIRE(pts, ld, cols, n_pts, n_frames, sc, u, valid);
    for (int64_t f = 0; f < n_frames; ++f) {
        uint32_t bins[SC_BINS];
        memset(bins, 0, sizeof bins);
        int64_t n = n_pts[f];
        if (n > ld) n = ld;
        for (int64_t p = 0; p < n; ++p) {
            const float *q = pts + (f * ld + p) * cols;
            int bin;
            uint32_t enc;
            if (sc_point(q[0], q[1], q[2], &bin, &enc) && enc > bins[bin]) bins[bin] = enc;
        }
        uint64_t m = 0;
        for (int col = 0; col < SC_SECTORS; ++col) {
            float v[SC_RINGS];
            for (int r = 0; r < SC_RINGS; ++r) sc[f * SC_BINS + r * SC_SECTORS + col] = v[r] = sc_decode(bins[r * SC_SECTORS + col]);
            if (sc_column(v, u + f * SC_BINS + col * SC_RINGS)) m |= 1ull << col;
        }
        valid[f] = m;
    }
    return CAELO_OK;
}

LC_API int caelo_host_loop_search(const float *u, const uint64_t *valid, int64_t n, int64_t q0, int64_t q1, int min_gap, int k,
                                     float max_dist, int min_cols, int32_t *cand, float *dist, int32_t *shift, float *dense_dist,
                                     int8_t *dense_shift) {
    LC_REQUIRE(u, valid, n, q0, q1, min_gap, k, max_dist, min_cols, cand, dist, shift, dense_dist, dense_shift);
    for (int64_t i = q0; i < q1; ++i) {
        int32_t *oc = cand + (i - q0) * k, *os = shift + (i - q0) * k;
        float *od = dist + (i - q0) * k;
        for (int t = 0; t < k; ++t) { oc[t] = -1; od[t] = __builtin_inff(); os[t] = -1; }
        if (dense_dist)
            for (int64_t j = 0; j < n; ++j) { dense_dist[(i - q0) * n + j] = __builtin_inff(); dense_shift[(i - q0) * n + j] = -1; }
        const float *ui = u + i * SC_BINS;
        for (int64_t j = 0; j <= i - min_gap; ++j) {
            const float *uj = u + j * SC_BINS;
            float bd = __builtin_inff();
            int bs = -1;
            for (int s = 0; s < SC_SECTORS; ++s) {
                if (__builtin_popcountll(valid[i] & lc_rot(valid[j], s)) < min_cols) continue;   // (lc_shift_dist would skip it)
                float num = 0.0f;
                const int head = SC_BINS - SC_RINGS * s;                                          // k + 20 s wraps at k = head
                for (int kk = 0; kk < head; ++kk) num = fmaf(ui[kk], uj[kk + SC_RINGS * s], num);
                for (int kk = head; kk < SC_BINS; ++kk) num = fmaf(ui[kk], uj[kk - head], num);
                float d;
                if (lc_shift_dist(num, valid[i], valid[j], s, min_cols, &d) && d < bd) { bd = d; bs = s; }
            }
            if (dense_dist && bs >= 0) { dense_dist[(i - q0) * n + j] = bd; dense_shift[(i - q0) * n + j] = (int8_t)bs; }
            if (bs < 0 || !(bd < max_dist)) continue;
            // ascending j: an equal distance never moves an earlier candidate
            int at = k;
            while (at > 0 && (oc[at - 1] < 0 || bd < od[at - 1])) --at;
            if (at == k) continue;
            for (int t = k - 1; t > at; --t) { oc[t] = oc[t - 1]; od[t] = od[t - 1]; os[t] = os[t - 1]; }
            oc[at] = (int32_t)j; od[at] = bd; os[at] = bs;
        }
    }
    return CAELO_OK;
}
