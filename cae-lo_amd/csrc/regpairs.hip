// regpairs.hip -- caelo_register_pairs: the pipeline's pair stage (NN match, RANSAC hypotheses, certificates, refit) over a TABLE of
// frame pairs whose rows are already resident, e.g. the frame steps 2, 5, 10 of a sequence after ONE extraction pass.
//
// Nothing is computed here that the consecutive path does not compute: match_set (match.hip) and ransac_set (ransac.hip) launch the pair
// stage's kernels over a caelo_pair_set per slice of the table, so a pair gives the bits it gives in a pipeline batch or through
// caelo_match + caelo_ransac.  What this file adds is the host side: the argument checks (the table and the key point counts are read
// back once, before any launch), the slice order, the slices' sets (slice_set) and the walk over the slices.
//
// Slice order: the table entries are sorted (stably) by (frame 0, frame 1) on the host while they are being checked, and a launch
// covers CAELO_FB_MAX consecutive entries of that order.  Pairs that share their frame 0 -- steps 1, 5 and 10 from one anchor --
// then sit in one launch, and the chain (a, a + s), (a + s, a + 2 s) has its shared frame in neighbouring slots: the second fetch
// of a frame's rows (262 KB) hits L2.  Outputs are indexed by the table entry, so the caller sees its own order.
// Host cost per call: ONE wait for the stream (the read-back of the table and of n_key, 8 B per pair + 4 B per frame), the sort, and
// three host vectors; nothing goes up -- a slice's pairs are part of its launches' arguments.
// caelo_register_pairs_desc: the same walk with the NN match on descriptors of the caller's ([n_frames][1024][ld_desc], up to 256
// wide) instead of the rows' columns 0:60; xyz and the counts still come from the rows.
// caelo_register_pairs_adaptive: the same checks and the same single wait, the match with the two frames exchanged, and the
// comparison protocol's registrar (adaptive.hip) over the whole table in one launch.
#include "caelo_internal.h"

#include <algorithm>
#include <vector>

namespace {
constexpr int64_t RP_ALIGN = 256;
inline int64_t rp_up(int64_t b) { return (b + RP_ALIGN - 1) / RP_ALIGN * RP_ALIGN; }
inline int64_t rp_match_stride(int dim = 60) { return rp_up(caelo_match_ws_bytes_dim(CAELO_MAX_KEYPTS, dim)); }
inline int64_t rp_ransac_stride() { return rp_up(caelo_ransac_ws_bytes()); }
}  // namespace

// CAELO_FB_MAX slots of match + RANSAC workspace, whatever the table's length (the slices reuse them)
CAELO_API int64_t caelo_register_pairs_ws_bytes(int64_t n_pairs) {
    if (n_pairs < 0) return 0;
    return CAELO_FB_MAX * (rp_match_stride() + rp_ransac_stride());
}

CAELO_API int64_t caelo_register_pairs_ws_bytes_dim(int64_t n_pairs, int dim) {
    if (n_pairs < 0) return 0;
    return CAELO_FB_MAX * (rp_match_stride(dim) + rp_ransac_stride());
}

// The table and the counts as the device holds them once `s` has reached the call: read back (ONE wait), checked, and the entries
// ordered (stably) by (frame 0, frame 1).  -> CAELO_OK, or the refusal with the error text set
static int read_table(int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs, hipStream_t s, std::vector<int32_t> &tab,
                      std::vector<int32_t> &order) {
    std::vector<int32_t> nk((size_t)n_frames);
    tab.resize((size_t)n_pairs * 2);
    order.resize((size_t)n_pairs);
    CAELO_HIP(hipMemcpyAsync(tab.data(), pairs, tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CAELO_HIP(hipMemcpyAsync(nk.data(), n_key, nk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CAELO_HIP(hipStreamSynchronize(s));
    for (int64_t q = 0; q < n_pairs; ++q)
        for (int side = 0; side < 2; ++side) {
            const int64_t f = tab[(size_t)(2 * q + side)];
            if (f < 0 || f >= n_frames) {
                caelo_set_error("caelo_register_pairs: pair %lld names frame %lld, outside [0, %lld)", (long long)q, (long long)f, (long long)n_frames);
                return CAELO_ERR_ARG;
            }
            if (nk[(size_t)f] < 1 || nk[(size_t)f] > CAELO_MAX_KEYPTS) {
                caelo_set_error("caelo_register_pairs: frame %lld of pair %lld has n_key %d, outside [1, %d]", (long long)f, (long long)q,
                                (int)nk[(size_t)f], CAELO_MAX_KEYPTS);
                return CAELO_ERR_ARG;
            }
        }
    for (int64_t q = 0; q < n_pairs; ++q) order[(size_t)q] = (int32_t)q;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return tab[2 * (size_t)a] != tab[2 * (size_t)b] ? tab[2 * (size_t)a] < tab[2 * (size_t)b] : tab[2 * (size_t)a + 1] < tab[2 * (size_t)b + 1];
    });
    return CAELO_OK;
}

// A table's pairs reach the kernels as the pipeline's do: a caelo_pair_set per slice, filled on the host from the table it has read
// back anyway.  PairSlices says where things lie -- the descriptors ([n_frames][1024][ld] f32: the rows' own columns 0:60 at ld 64, or
// the caller's block), the outputs (indexed by table entry; null where a caller has none) and the workspace slots (indexed by slot).
struct PairSlices {
    const float *rows, *desc;
    const int32_t *n_key;
    int64_t ld_desc;
    bool exchanged;   // the match takes frame 1 of an entry as its frame 0 (the adaptive registrar: argmin over frame b)
    int64_t *pair_idx;
    const double *rand;
    caelo_pose_result *result;
    uint8_t *mask;
    caelo_ransac_cert *cert;
    int32_t cert_only, *faults;
    char *ws_match, *ws_ransac;
    int64_t ws_match_stride, ws_ransac_stride;
};
// slot z of the slice at q0 is entry order[q0 + z] of the table's host copy `tab`; ONE set serves both launches: f0 / f1 / n0 / n1 / pair_idx / ws_match are the
// match's, pc0 / pc1 (the rows' xyz columns of frames 0 and 1, never exchanged) and the rest are RANSAC's
static caelo_pair_set slice_set(const PairSlices &t, const std::vector<int32_t> &tab, const std::vector<int32_t> &order, int64_t q0) {
    caelo_pair_set ps = {};
    ps.n = (int32_t)std::min<int64_t>(CAELO_FB_MAX, (int64_t)order.size() - q0);
    ps.faults = t.faults;
    for (int z = 0; z < ps.n; ++z) {
        const int64_t q = order[(size_t)(q0 + z)], a = tab[(size_t)(2 * q)], b = tab[(size_t)(2 * q + 1)];
        const int64_t m0 = t.exchanged ? b : a, m1 = t.exchanged ? a : b;
        caelo_pair_dev &d = ps.p[z];
        d.f0 = t.desc + m0 * (CAELO_MAX_KEYPTS * t.ld_desc); d.f1 = t.desc + m1 * (CAELO_MAX_KEYPTS * t.ld_desc);
        d.n0 = t.n_key + m0; d.n1 = t.n_key + m1;
        d.pc0 = t.rows + a * ((int64_t)CAELO_MAX_KEYPTS * 64) + 60; d.pc1 = t.rows + b * ((int64_t)CAELO_MAX_KEYPTS * 64) + 60;
        d.pair_idx = t.pair_idx + q * CAELO_MAX_KEYPTS;
        d.ws_match = t.ws_match + (int64_t)z * t.ws_match_stride;
        d.ws_ransac = t.ws_ransac ? t.ws_ransac + (int64_t)z * t.ws_ransac_stride : nullptr;
        d.rand = t.rand ? t.rand + q * ((int64_t)CAELO_RANSAC_LEVELS * CAELO_RANSAC_MAX_TRIALS * 4) : nullptr;
        d.result = t.result ? t.result + q : nullptr;
        d.mask = t.mask ? t.mask + q * CAELO_MAX_KEYPTS : nullptr;
        d.cert = t.cert ? t.cert + q : nullptr;
        d.cert_only = t.cert_only;
    }
    return ps;
}

// The NN match on `desc` (the rows themselves at ld 64, 60 wide, or the caller's block): match_set launches whichever match kernels
// `dim` selects.  RANSAC never reads a descriptor.
static int register_pairs(caelo_ctx *c, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs,
                          const double *rand, int64_t *pair_idx_out, caelo_pose_result *results_out, uint8_t *masks_out,
                          caelo_ransac_cert *certs_out, void *ws, void *stream, const float *desc, int64_t ld_desc, int dim) {
    CAELO_REQUIRE(pairs, "null pair table");
    CAELO_REQUIRE(n_frames >= 1 && n_frames < (1LL << 31), "n_frames must lie in [1, 2^31)");
    CAELO_REQUIRE(n_pairs >= 0 && n_pairs < (1LL << 31), "n_pairs must lie in [0, 2^31)");
    CAELO_REQUIRE(c && rows && n_key && rand && pair_idx_out && ws, "null argument");
    CAELO_REQUIRE((results_out && masks_out) || (certs_out && !results_out && !masks_out),
                  "results_out and masks_out go together; without them certs_out must take the pairs' certificates");
    CAELO_REQUIRE((((uintptr_t)rows) & 15u) == 0 && (((uintptr_t)certs_out) & 15u) == 0 && (((uintptr_t)masks_out) & 3u) == 0 &&
                      (((uintptr_t)ws) & 15u) == 0,
                  "rows, certs_out and ws must be 16-byte aligned, masks_out 4-byte aligned");
    if (n_pairs == 0) return CAELO_OK;
    hipStream_t s = caelo_stream(stream);
    std::vector<int32_t> tab, order;
    if (const int rc = read_table(n_frames, n_key, pairs, n_pairs, s, tab, order)) return rc;
    PairSlices t = {};
    t.rows = rows; t.n_key = n_key; t.desc = desc; t.ld_desc = ld_desc;
    t.pair_idx = pair_idx_out; t.rand = rand; t.result = results_out; t.mask = masks_out; t.cert = certs_out;
    t.cert_only = results_out ? 0 : 1;
    t.ws_match_stride = rp_match_stride(dim); t.ws_ransac_stride = rp_ransac_stride();
    t.ws_match = (char *)ws;
    t.ws_ransac = t.ws_match + CAELO_FB_MAX * t.ws_match_stride;
    t.faults = c->faults;
    for (int64_t q0 = 0; q0 < n_pairs; q0 += CAELO_FB_MAX) {   // the slot workspaces are reused slice after slice: the stream orders them
        const caelo_pair_set ps = slice_set(t, tab, order, q0);
        int rc = match_set(ps, (int)ld_desc, CAELO_MAX_KEYPTS, (int)ld_desc, CAELO_MAX_KEYPTS, dim, s);
        if (rc == CAELO_OK) rc = ransac_set(ps, 64, 64, CAELO_MAX_KEYPTS, s);
        if (rc) return rc;
    }
    return CAELO_OK;
}

CAELO_API int caelo_register_pairs(caelo_ctx *c, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs,
                                   const double *rand, int64_t *pair_idx_out, caelo_pose_result *results_out, uint8_t *masks_out,
                                   caelo_ransac_cert *certs_out, void *ws, void *stream) {
    return register_pairs(c, rows, n_frames, n_key, pairs, n_pairs, rand, pair_idx_out, results_out, masks_out, certs_out, ws, stream, rows, 64, 60);
}

CAELO_API int caelo_register_pairs_desc(caelo_ctx *c, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs,
                                        const double *rand, int64_t *pair_idx_out, caelo_pose_result *results_out, uint8_t *masks_out,
                                        caelo_ransac_cert *certs_out, void *ws, void *stream, const float *desc, int64_t ld_desc, int dim) {
    CAELO_REQUIRE(desc, "null descriptors");
    CAELO_REQUIRE(dim >= 1 && dim <= 256 && ld_desc >= dim && ld_desc < (1LL << 31), "dim must lie in [1, 256] and ld_desc in [dim, 2^31)");
    return register_pairs(c, rows, n_frames, n_key, pairs, n_pairs, rand, pair_idx_out, results_out, masks_out, certs_out, ws, stream, desc, ld_desc, dim);
}

// ---- the comparison protocol's registrar over a table (adaptive.hip; include/caelo.h) ----------------------------------------------
// The match is match_set's with the two frames EXCHANGED (for each point of frame a the nearest descriptor of frame b), slice after
// slice on CAELO_FB_MAX workspace slots; then one launch registers every entry.  Nothing but the match needs a workspace.
CAELO_API int64_t caelo_register_pairs_adaptive_ws_bytes(int64_t n_pairs, int dim) {
    if (n_pairs < 0) return 0;
    return CAELO_FB_MAX * rp_match_stride(dim);
}

CAELO_API int caelo_register_pairs_adaptive(caelo_ctx *c, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs,
                                            int64_t n_pairs, const double *draws, double threshold, int64_t *pair_idx_out,
                                            caelo_adaptive_result *results_out, uint8_t *masks_out, void *ws, void *stream, const float *desc,
                                            int64_t ld_desc, int dim) {
    CAELO_REQUIRE(pairs, "null pair table");
    CAELO_REQUIRE(n_frames >= 1 && n_frames < (1LL << 31), "n_frames must lie in [1, 2^31)");
    CAELO_REQUIRE(n_pairs >= 0 && n_pairs < (1LL << 31), "n_pairs must lie in [0, 2^31)");
    CAELO_REQUIRE(c && rows && n_key && draws && pair_idx_out && results_out && masks_out && ws, "null argument");
    CAELO_REQUIRE((((uintptr_t)rows) & 15u) == 0 && (((uintptr_t)ws) & 15u) == 0 && (((uintptr_t)results_out) & 7u) == 0 && (((uintptr_t)draws) & 7u) == 0,
                  "rows and ws must be 16-byte aligned, results_out and draws 8-byte aligned");
    if (!desc) { desc = rows; ld_desc = 64; dim = 60; }
    CAELO_REQUIRE(dim >= 1 && dim <= 256 && ld_desc >= dim && ld_desc < (1LL << 31), "dim must lie in [1, 256] and ld_desc in [dim, 2^31)");
    if (n_pairs == 0) return CAELO_OK;
    hipStream_t s = caelo_stream(stream);
    std::vector<int32_t> tab, order;
    if (const int rc = read_table(n_frames, n_key, pairs, n_pairs, s, tab, order)) return rc;
    PairSlices t = {};
    t.rows = rows; t.n_key = n_key; t.desc = desc; t.ld_desc = ld_desc; t.exchanged = true;
    t.pair_idx = pair_idx_out; t.ws_match = (char *)ws; t.ws_match_stride = rp_match_stride(dim);
    t.faults = c->faults;
    for (int64_t q0 = 0; q0 < n_pairs; q0 += CAELO_FB_MAX)
        if (const int rc = match_set(slice_set(t, tab, order, q0), (int)ld_desc, CAELO_MAX_KEYPTS, (int)ld_desc, CAELO_MAX_KEYPTS, dim, s)) return rc;
    caelo_adaptive_table at = {};
    at.rows = rows; at.n_key = n_key; at.pairs = pairs; at.pair_idx = pair_idx_out; at.draws = draws; at.threshold = threshold;
    at.result = results_out; at.mask = masks_out; at.n_pairs = n_pairs;
    return adaptive_table(at, s);
}
