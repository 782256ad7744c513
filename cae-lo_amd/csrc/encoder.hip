// encoder.hip -- 3D-CAE voxel-patch descriptor encoder on the gfx950 matrix cores (f32 in / out / accumulate).
//
// Reference behaviour restated here (never its code): PatchEncoder.predict via
// GetFeaturesFromPatches (Match.py:130-135) with the shipped EncoderModel4VoxelPatch.h5:
//   Conv3D(1->8,3^3,same) tanh -> MaxPool3D(2) -> Conv3D(8->16) tanh -> MaxPool3D(2)
//   -> Conv3D(16->32) tanh -> Flatten(x,y,z,c) -> Dense(200) tanh -> Dense(20) tanh
// (Keras channels-last, zero 'same' padding, cross-correlation).  The training script AE4VoxelPatch.py:177-197 builds the same stack
// with relu on the four hidden layers and a linear code: the kernel bodies are templates over the activation, the kernels named
// below are their tanh instantiation and the _relu / _act siblings (k_enc_stage1_relu, k_enc_bgo_table_relu, k_enc_stage1x_relu,
// k_enc_conv3_relu, k_enc_head_mfma_act<.., H, C>; Dense(200) has no activation of its own) serve such a model
// (caelo_set_encoder_model).  7.905 MFLOP per patch, 24.28 GFLOP per 3072-patch frame.
//
// Arithmetic: every f32 product of conv1, conv2, conv3 and Dense(200) runs on the f16 matrix pipe (v_mfma_f32_16x16x32_f16) from
// 2-way operand splits x = hi + lo (enc_common.h), accumulated in f32.  Stage 1 sums all four partial products; conv3 and Dense(200)
// sum three, lo hi + hi lo + hi hi, smallest first (the dropped lo lo term is 2^-22 relative).  Dense(20) is an exact f32 fmaf chain
// on v_mfma_f32_16x16x4_f32.  All tanh are enc_tanh (v_exp_f32 + v_rcp_f32, |err| < 6e-7).
//
// One translation unit, a file per stage (each with the host builder of its kernel's weight operand), launched in this order by
// encode_batch_impl below:
//   enc_stage1x.inc  k_enc_stage1x<COUNT>: persistent workgroups, a patch at a time from eight per-XCD queues; conv1 + pool1 as a
//                    GEMM over the receptive-field masks of the non-empty cells, conv2 on the difference to the background response
//                    with all-background rows skipped exactly, pool2 -> P2 [patch][4][4][4][16] (4 KB).  k_enc_bgo_table: the outputs
//                    of an all-background tile pair, once per model.
//   enc_stage1.inc   k_enc_stage1: the same layers with f32-input MFMAs and conv1 on the VALU -- the PRECISION REFERENCE the f16 x 2
//                    stage 1 is measured against, chosen per context by caelo_set_encoder_reference.
//   enc_conv3.inc    k_enc_conv3: implicit GEMM, 2 patches per workgroup, the W3 n-tile resident in 112 VGPRs, P2 split while staged
//                    in LDS, two taps per MFMA, zero halo planes skipped -> F3 [patch][2048].
//   enc_dense1.inc   k_enc_dense1p<K, MTW>: split-K GEMM [rows, K] x [K, 208], 64 / 128 / 192-row tiles, one workgroup per CU,
//                    host-built weight stages moved by LDS-DMA through three buffers, rows split into LDS; K = 2048 here, 16384 for
//                    the 32^3 case (config5.hip).
//   enc_head.inc     k_enc_head_mfma<SPLIT>: k slices in order + bias + tanh, Dense(20) + tanh of 16 patches per workgroup, written
//                    into each frame's rows (the patches of several frames can share one launch set).
//   enc_model.inc    caelo_set_encoder_model and its siblings: the range guard, the plain copies, every operand image.
// This file keeps what they share -- enc_act, the work-item helpers, the counter constants -- the workspace layout, the launch sequence,
// the C ABI entry points and the hooks of the 32^3 case.
#include <math.h>

#include "enc_common.h"
#include <vector>
#include <stdlib.h>
#include <string.h>

// The activation of a layer as a template argument (CAELO_ACT_*): the hidden layers' H in {tanh, relu}, the code's C in {tanh,
// linear}.  relu and the identity are monotone like tanh, so pooling the pre-activations stays exact: relu(max) == max(relu) bit for
// bit.  relu is fmaxf(x, 0.0f): +0.0 for every negative pre-activation.
template <int ACT>
__device__ __forceinline__ float enc_act(float x) {
    if (ACT == CAELO_ACT_RELU) return fmaxf(x, 0.0f);
    if (ACT == CAELO_ACT_LINEAR) return x;
    return enc_tanh(x);
}
// the same on the host, for the background vector bg = act(b1) of the C0 table (relu: the bits the device's fmaxf gives)
static float enc_act_host(int act, float x) {
    return act == CAELO_ACT_RELU ? fmaxf(x, 0.0f) : (act == CAELO_ACT_LINEAR ? x : tanhf(x));
}

#define DENSE_N 200
#define DENSE_NP 208  // padded to 13 MFMA n-tiles
#define DENSE_K 2048
// Counters in the workspace header (caelo_internal.h: CAELO_ENC_WS_*), each on a 128-byte line of its own: int 0 = k_enc_stage1's work
// counter, ints 256 + 32 x = stage 1x's eight per-XCD queues, ints 512 + 32 x = conv3's eight ticket counters.  Stage 1 zeroes conv3's, conv3 both of stage 1's.
#define ENC_XCD_CSTRIDE 32   // ints between two per-XCD work counters (one 128-byte line each)
#define C3X_TICKET_INT 512   // conv3's eight per-XCD ticket counters: ints 512 + 32 x of the workspace header (bytes 2048 + 128 x)

// phase timestamps (100 MHz) of workgroup 0's first patch in the last k_enc_stage1 launch (debug aid); the PROF=1 / C3PROF=1 builds
// accumulate their phase cycles here instead (enc_stage1.inc, enc_stage1x.inc, enc_conv3.inc)
__device__ unsigned long long g_enc_stamp[16];
int enc_debug_copy(unsigned long long *out_host) {
    CAELO_HIP(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_enc_stamp), sizeof(unsigned long long) * 16));
    return CAELO_OK;
}
#define S1_XDEAL(YI) ((YI) == 0 ? 0 : ((YI) == 1 ? 3 : ((YI) == 2 ? 1 : 2)))  // both stage-1 kernels' deal of tile pairs to wavefronts

// Work item J of a launch -> where its bits are and which output row it fills.  J is wave-uniform: everything here
// stays in scalar registers (the per-frame counts come through the scalar cache).
__device__ inline int enc_items_total(const caelo_enc_in &in, int64_t n_patches) {
    if (!in.dedup) return (int)n_patches;
    int acc = 0;
    for (int f = 0; f < in.n_frames; ++f) acc += enc_tables(in, f)->count;
    return acc;
}
__device__ inline int enc_item_row(const caelo_enc_in &in, int J, int &f, int &i) {  // de-duplicated launch
    f = 0;
    i = J;
    while (f + 1 < in.n_frames) {
        const int c = enc_tables(in, f)->count;
        if (i < c) break;
        i -= c;
        ++f;
    }
    return f * in.per_frame + i;
}
__device__ inline void enc_item(const caelo_enc_in &in, int J, int nk, int group, const unsigned long long *&src, int &row) {
    if (in.dedup) {
        int f, i;
        row = enc_item_row(in, J, f, i);
        src = in.bits + (size_t)f * in.frame_stride + (size_t)enc_tables(in, f)->list[i] * 64;
    } else {
        row = (J % nk) * group + (group - 1 - J / nk);  // coarsest scale first
        src = in.bits + (size_t)row * 64;
    }
}

#include "enc_stage1.inc"
#include "enc_stage1x.inc"
#include "enc_conv3.inc"
#include "enc_dense1.inc"
#include "enc_head.inc"
#include "enc_model.inc"

// ------------------------------------------------------------------------------------------------
// host entry
// ------------------------------------------------------------------------------------------------
static inline int64_t pad64(int64_t n) { return (n + D1_BM - 1) / D1_BM * D1_BM; }  // rows padded to whole dense-1 tiles

// resident workgroup slots of the 256-thread kernel K on this device = the size of its persistent grid; asked once per device
// (per_device_once: caelo_internal.h), FALLBACK where the runtime will not say
template <auto K, int FALLBACK>
static int enc_resident_slots(int device) {
    static int slot[CAELO_MAX_DEVICES];
    static bool have[CAELO_MAX_DEVICES];
    static std::mutex mu;
    return per_device_once(device, slot, have, mu, [&] {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)K, 256, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || per_cu * cus <= 0)
            return FALLBACK;
        return per_cu * cus;
    });
}

CAELO_API int64_t caelo_encode_ws_bytes(int64_t n_patches) {
    const int64_t np = pad64(n_patches);
    return CAELO_ENC_WS_HEADER + (np * 1024 + np * 2048 + (int64_t)D1_SPLIT * np * DENSE_NP) * (int64_t)sizeof(float);
}

CAELO_API int caelo_encode_ws_layout(int64_t n_patches, int64_t out[6]) {
    CAELO_REQUIRE(out && n_patches > 0, "caelo_encode_ws_layout: bad argument");
    const int64_t np = pad64(n_patches);
    out[0] = CAELO_ENC_WS_HEADER;
    out[1] = out[0] + np * 1024 * (int64_t)sizeof(float);
    out[2] = out[1] + np * 2048 * (int64_t)sizeof(float);
    out[3] = np;
    out[4] = D1_SPLIT_OF(DENSE_K);
    out[5] = D1_SPLIT;
    return CAELO_OK;
}

int encode_impl(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                       void *ws, hipStream_t s, hipEvent_t *ev /* 5 events or null */) {
    CAELO_REQUIRE(out, "null argument");
    caelo_enc_out outs;
    outs.base[0] = out;
    outs.per_frame = n_patches > 0 ? n_patches : 1;
    return encode_batch_impl(c, bits, n_patches, group, outs, out_stride, ws, s, ev);
}

int encode_batch_impl(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, const caelo_enc_out &outs,
                      int out_stride, void *ws, hipStream_t s, hipEvent_t *ev /* 5 events or null */, const caelo_enc_in *in) {
    CAELO_REQUIRE(c && bits && ws, "null argument");
    // plain launch: every patch, contiguous
    const caelo_enc_in ein = in ? *in : caelo_enc_in{(const unsigned long long *)bits, 0, (int32_t)(n_patches < 0x7FFFFFFF ? n_patches : 0), 1, 0, 0};
    CAELO_REQUIRE(!ein.dedup || (ein.n_frames >= 1 && ein.n_frames <= CAELO_ENC_MAX_FRAMES && ein.per_frame % (3 * D1_BM) == 0 &&
                                 (int64_t)ein.n_frames * ein.per_frame == n_patches),
                  "bad de-duplicated launch");
    CAELO_REQUIRE(outs.per_frame > 0 && (n_patches + outs.per_frame - 1) / outs.per_frame <= CAELO_ENC_MAX_FRAMES, "bad frame table");
    // (the de-duplication tables address representatives by row of the launch set = frame * 3072 + position: dedup.hip)
    CAELO_REQUIRE(!ein.dedup || ein.per_frame == CAELO_FRAME_PATCHES, "de-duplicated launches hold whole frames of 3072 patches");
    CAELO_REQUIRE(c->has_enc, "encoder weights not set (caelo_set_encoder_weights)");
    CAELO_REQUIRE(n_patches > 0 && n_patches < 0x7FFFFFFF && group >= 1 && out_stride >= group * 20, "bad shape");
    const int64_t np = pad64(n_patches);
    // ws = [header (CAELO_ENC_WS_HEADER bytes): work counter, zero between calls (the owner zero-fills ws once, conv3 resets it); bytes 3072..4095
    // = MFMA instructions the last profiled stage-1 launch executed, eight partial counts] | P2 | F3 | dense-1 partial sums
    int *work_counter = (int *)ws;
    unsigned long long *mfma_count = (unsigned long long *)((char *)ws + CAELO_ENC_WS_MFMA);   // eight counters, a 128-byte line each
    float *p2 = (float *)((char *)ws + CAELO_ENC_WS_HEADER);
    float *f3 = p2 + np * 1024;
    float *part = f3 + np * 2048;
    if (np > n_patches)  // rows of the last 64-row tile that no patch writes
        CAELO_HIP(hipMemsetAsync(f3 + n_patches * 2048, 0, (size_t)(np - n_patches) * 2048 * sizeof(float), s));
    // persistent grid = exactly the resident workgroup slots (weights stay in registers across patches,
    // no second partially filled round)
    // Stage 1 = k_enc_stage1x (enc_stage1x.inc: conv1 on the matrix cores, f16 x 2 products, three 168-register workgroups per CU).
    // The exact-f32 k_enc_stage1 of round 2 stays as the PRECISION REFERENCE, chosen per context by caelo_set_encoder_reference --
    // never by the environment: the library reads no variable that changes arithmetic.  (The kernels rounds 1-3 measured and lost
    // with -- one wavefront per patch, conv1 / conv2 as two kernels, the two-barrier Dense(200), the one-patch-per-wavefront head, the
    // VALU response layer, the all-f64 match as a default -- are gone from the library; DESIGN.md 4 keeps their numbers.)
    const bool stage1x = !c->enc_reference;
    const bool relu = c->enc_hidden == CAELO_ACT_RELU;   // the relu siblings have their tanh kernels' registers, LDS and occupancy
    const int slots1x = enc_resident_slots<k_enc_stage1x<false>, 512>(c->device);
    int *xcd_counters = (int *)((char *)ws + 1024);  // 8 x one 128-byte line
    const int slots1 = enc_resident_slots<k_enc_stage1, 768>(c->device);   // 3 workgroups on each of MI355X's 256 CUs
    // Inside the frame pipeline the persistent grids leave a fifth (stage 1) / a quarter (conv3) of their slots free: stage 1 and
    // conv3 otherwise own every register file for their whole run and the other streams' kernels only get CUs between them
    // (round 1: +3 % frames/s; with the round-2 executor the setting is worth about 1 %, caelo_enc_in::yield bits)
    const int64_t cap1 = (ein.yield & 1) ? (int64_t)slots1 * 4 / 5 : slots1;
    const unsigned g1 = (unsigned)(n_patches < cap1 ? n_patches : cap1);
    if (ev) CAELO_HIP(hipEventRecord(ev[0], s));
    const int order_group = (n_patches % group == 0) ? group : 1;
    if (stage1x) {
        // CAELO_S1X_SLOTS: grid size by hand (measurement: 128 / 256 / 384 / 512 workgroups take 692 / 376 / 281 / 233 us per 24 576
        // patches -- a workgroup alone on its CU needs 3.9 us per patch, two sharing one 4.85 us each: latency bound)
        static const int slots_env = getenv("CAELO_S1X_SLOTS") ? atoi(getenv("CAELO_S1X_SLOTS")) : 0;
        // inside the pipeline (yield bit 0): two of the three workgroups a CU can hold -- the third's registers and LDS go to the front
        // and pair kernels of the other streams (frames/s at 120 batches against the grid: 448 / 512 / 576 / 640 / 704 / 768 workgroups
        // = 20.0 / 20.4 / 20.2 / 19.6 / 19.2 / 17.8 k, profiles/r04_pipe_sweep.txt); alone, all three (207 against 248 us)
        const int64_t capx = slots_env > 0 ? slots_env : ((ein.yield & 1) ? (int64_t)slots1x * 2 / 3 : slots1x);
        unsigned gx = (unsigned)(n_patches < capx ? n_patches : capx);
        // a by-hand grid below eight workgroups would leave the queues gridDim.x .. 7 without a workgroup (item j belongs to queue
        // j % 8, block b serves queue b % 8 only): their patches would keep stale P2 without any error.  The default grid has at
        // least eight workgroups whenever the launch has eight items.
        if (slots_env > 0 && gx < 8u && n_patches >= 8) gx = 8u;
        if (ev) {   // profiling calls count the MFMAs the kernel executes (bench.py's roofline); same code otherwise
            CAELO_HIP(hipMemsetAsync(mfma_count, 0, 1024, s));
            CAELO_HIP(hipEventRecord(ev[0], s));
        }
        const auto k1x = ev ? (relu ? k_enc_stage1x_relu<true> : k_enc_stage1x<true>) : (relu ? k_enc_stage1x_relu<false> : k_enc_stage1x<false>);
        k1x<<<gx, 256, 0, s>>>(ein, n_patches, order_group, work_counter, (const uint4 *)c->enc_w1f, c->enc_b1, (const uint4 *)c->enc_w2x,
                               c->enc_c0, p2, mfma_count);
        CAELO_LAUNCH_CHECK();
    } else {
        if (ev) CAELO_HIP(hipMemsetAsync(mfma_count, 0, 1024, s));   // (the f32 kernel has no register left to count)
        const auto k1 = relu ? k_enc_stage1_relu : k_enc_stage1;
        k1<<<g1, 256, 0, s>>>(ein, n_patches, order_group, work_counter, c->enc_w1, c->enc_b1, c->enc_w2, c->enc_c0, p2);
        CAELO_LAUNCH_CHECK();
    }
    if (ev) CAELO_HIP(hipEventRecord(ev[1], s));
    const int64_t pairs = (n_patches + 1) / 2;
    const int64_t cap3 = ((ein.yield & 2) ? 256 : ((ein.yield & 4) ? 384 : 512)) * C3X_WGS / 2;
    const unsigned g3 = (unsigned)(pairs < cap3 ? pairs : cap3);  // persistent: two 4-wave workgroups per CU
    const auto k3 = relu ? k_enc_conv3_relu : k_enc_conv3;
    k3<<<g3, 256, 0, s>>>(p2, n_patches, ein, (const uint4 *)c->enc_w3x, c->enc_b3, f3, work_counter, xcd_counters);
    CAELO_LAUNCH_CHECK();
    if (ev) CAELO_HIP(hipEventRecord(ev[2], s));
    {
        const int rc = dense1_launch<DENSE_K>(c->device, f3, np, c->enc_wd1x, part, ein, s);
        if (rc) return rc;
    }
    if (ev) CAELO_HIP(hipEventRecord(ev[3], s));
    {
        constexpr int SP = D1_SPLIT_OF(DENSE_K);
        const dim3 gh((unsigned)((n_patches + 15) / 16));
        const bool linear = c->enc_code == CAELO_ACT_LINEAR;
        const auto kh = relu ? (linear ? k_enc_head_mfma_act<SP, CAELO_ACT_RELU, CAELO_ACT_LINEAR> : k_enc_head_mfma_act<SP, CAELO_ACT_RELU, CAELO_ACT_TANH>)
                             : (linear ? k_enc_head_mfma_act<SP, CAELO_ACT_TANH, CAELO_ACT_LINEAR> : k_enc_head_mfma<SP>);
        kh<<<gh, 256, 0, s>>>(part, n_patches, np, c->enc_bd1, (const float4 *)c->enc_wd2q, c->enc_bd2, group, outs, out_stride, ein, c->faults);
    }
    CAELO_LAUNCH_CHECK();
    if (ev) CAELO_HIP(hipEventRecord(ev[4], s));
    return CAELO_OK;
}

// Dense(200) + Dense(20) of the 32^3 stress case (config5.hip): the same two kernels over K = 16384
int64_t enc_dense_pad(int64_t n) { return pad64(n); }
int64_t enc_dense32_part_bytes(int64_t np) { return (int64_t)D1_SPLIT * np * DENSE_NP * (int64_t)sizeof(float); }
void enc_dense32_slices(int64_t *used, int64_t *sized) {
    *used = D1_SPLIT_OF(16384);
    *sized = D1_SPLIT;
}
int enc_dense32_head_launch(caelo_ctx *c, const float *f3, int64_t n_patches, int64_t np, float *part, int group, float *out,
                            int out_stride, hipStream_t s) {
    const caelo_enc_in plain = {nullptr, 0, (int32_t)n_patches, 1, 0, 0};
    {
        const int rc = dense1_launch<16384>(c->device, f3, np, c->enc32_wd1x, part, plain, s);
        if (rc) return rc;
    }
    caelo_enc_out outs = {};
    outs.base[0] = out;
    outs.per_frame = n_patches;
    k_enc_head_mfma<D1_SPLIT_OF(16384)><<<(unsigned)((n_patches + 15) / 16), 256, 0, s>>>(part, n_patches, np, c->enc32_bd1, (const float4 *)c->enc_wd2q,
                                                                                     c->enc_bd2, group, outs, out_stride, plain, c->faults);
    CAELO_LAUNCH_CHECK();
    return CAELO_OK;
}

CAELO_API int caelo_encode(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, float *out,
                           int out_stride, void *ws, void *stream) {
    return encode_impl(c, bits, n_patches, group, out, out_stride, ws, caelo_stream(stream), nullptr);
}

// Same launches as caelo_encode with a HIP event between kernels on the launch stream; synchronises and
// returns the four kernel durations in ms (stage1, conv3, dense1, head).  Measurement aid for bench.py.
CAELO_API int caelo_encode_profile(caelo_ctx *c, const uint64_t *bits, int64_t n_patches, int group, float *out,
                                   int out_stride, void *ws, void *stream, float *ms_host) {
    CAELO_REQUIRE(ms_host != nullptr, "null argument");
    hipStream_t s = caelo_stream(stream);
    enc_prof_events pe;
    CAELO_HIP(pe.create());
    hipEvent_t *ev = pe.ev;
    int rc = encode_impl(c, bits, n_patches, group, out, out_stride, ws, s, ev);
    if (rc == CAELO_OK) {
        CAELO_HIP(hipEventSynchronize(ev[4]));
        for (int i = 0; i < 4; ++i) CAELO_HIP(hipEventElapsedTime(&ms_host[i], ev[i], ev[i + 1]));
        unsigned long long rows = 0, part[128];  // MFMA instructions executed, counted by the kernel itself (eight partial counts, a line each)
        CAELO_HIP(hipMemcpy(part, (char *)ws + CAELO_ENC_WS_MFMA, sizeof(part), hipMemcpyDeviceToHost));
        for (int i = 0; i < 8; ++i) rows += part[16 * i];
        // the f32 kernel counts tap rows (6 v_mfma_f32_16x16x4_f32 each), k_enc_stage1x its v_mfma_f32_16x16x32_f16 instructions
        const bool f32_kernel = c->enc_reference;   // (it does not count: 0 MFMAs reported)
        ms_host[4] = (float)((double)rows * (f32_kernel ? 6.0 : 1.0) / 1e6);
        ms_host[5] = f32_kernel ? 2.0f * 16 * 16 * 4 : 2.0f * 16 * 16 * 32;   // FLOPs of one counted instruction
    }
    return rc;
}

// The exact-f32 stage 1 of round 2 (k_enc_stage1: f32-input MFMAs for conv2, conv1 on the VALU) as this context's stage 1: the
// precision reference the f16 x 2 kernel is measured against (tests, tools/enc_layer_errors.py).  Slower (346 vs 224 us per
// 24 576 patches); everything behind stage 1 is unchanged.
CAELO_API int caelo_set_encoder_reference(caelo_ctx *c, int on) {
    CAELO_REQUIRE(c, "null argument");
    c->enc_reference = on != 0;
    return CAELO_OK;
}
