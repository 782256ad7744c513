/*
 * caelo.h -- C ABI of libcaelo.so, the MI355X-native (gfx950, HIP) CAE-LO feature-and-matching
 * engine.  The reference (SRainGit/CAE-LO) has no FFI: its boundary is a set of module-level
 * Python functions on NumPy arrays.  Each entry point below replaces the
 * device work behind one of those functions; caelo/api.py (ctypes) keeps the Python names,
 * argument order and return tuples.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer unless the name ends in _host; the caller owns all
 *     buffers (torch allocates them); no hidden allocation outside caelo_create /
 *     caelo_voxmap_create / caelo_set_*_weights;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 on success, negative caelo_status otherwise; caelo_last_error() gives text;
 *   - data-dependent conditions the reference reports as Python exceptions are written to a
 *     device-side int32 status word (CAELO_ST_* bit flags) so no call forces a host sync.
 */
#ifndef CAELO_H
#define CAELO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAELO_ABI_VERSION 6   /* 6: caelo_pipeline_run_uploading takes a copy table (copy_first: the copies of each batch); the device-side waits of the input side (wait_stream, the release of scans) are removed; 5: caelo_host_unbind_blas / _blas_probe / _bound_violations, caelo_host_random_sample, caelo_seqloader_*, caelo_patches_many, caelo_pipeline_run_uploading; 4: caelo_voxmap_export never waits for the device (a count above capacity is the overflow report), caelo_voxmap_order; 3: certificates, caelo_host_* */

/* geometry fixed by the reference: SphericalRing.py:28-58, Voxel.py:15-52 */
#define CAELO_RING_H 69
#define CAELO_RING_W 1800
#define CAELO_RING_C 5
#define CAELO_NET_H 64
#define CAELO_NET_W 1792
#define CAELO_RESP_C 8
#define CAELO_MAX_KEYPTS 1024
#define CAELO_PATCH_WORDS 64 /* 16^3 bits = 64 x u64, bit ((iy&3)*16+iz) of word (ix*4+iy/4) */
#define CAELO_DESC_DIM 20    /* per scale; 3 scales -> 60 */
#define CAELO_RANSAC_MAX_TRIALS 500
#define CAELO_RANSAC_LEVELS 3

typedef enum {
    CAELO_OK = 0,
    CAELO_ERR_ARG = -1,     /* bad argument (shape, null pointer, missing weights) */
    CAELO_ERR_HIP = -2,     /* a HIP runtime call failed */
    CAELO_ERR_CAPACITY = -3 /* voxel map too small for the cloud */
} caelo_status;

/* device-side status bits (int32 word, OR-ed by kernels) */
#define CAELO_ST_COL_OOB 1        /* a point projects to column 1800: IndexError at SphericalRing.py:91 */
#define CAELO_ST_VOXEL_OOB 2      /* voxel index outside its block: IndexError at Voxel.py:139 */
#define CAELO_ST_MAP_FULL 4       /* voxel hash table overflow: the cloud holds more bricks than a table of the map has slots (scale 0:
                                    one per point of max_points; scales 1 / 2: a quarter / a sixteenth of that).  The frame's voxels, patches
                                    and rows are unspecified; the map itself stays usable -- the next build on it, of either kind, gives what
                                    a new map gives -- and a caller retries the frame with a larger map */
#define CAELO_ST_FEW_VOXELS 8     /* a scale holds < 496 voxels: sklearn ValueError at Voxel.py:195-196 */
#define CAELO_ST_FEW_KEYPTS 16    /* K <= 50: assert at SphericalRing.py:286 */
#define CAELO_ST_NONFINITE 32     /* a NaN coordinate: int(nan) raises ValueError at SphericalRing.py:86-88 / Voxel.py:122-124 (an
                                   * infinite one is a point like any other there: dropped by range / row test or kept) */
#define CAELO_EXTRACT_EXACT_VOXELS 1 /* caelo_extract mode bit: the two-pass first-touch voxelization of caelo_voxelize
                                        (Voxel.py:139-141) instead of the one-pass build; both give the reference's voxel
                                        sets on every input, points on voxel faces included (tests compare them) */
#define CAELO_EXTRACT_NO_DEDUP 2     /* caelo_extract mode bit: encode every patch, also bit-identical copies of another one
                                        (by default equal patches of a frame are encoded once: same descriptors, bit for bit) */
#define CAELO_EXTRACT_EXACT_PATCHES 4 /* caelo_extract / caelo_frame_job.mode bit: GetPatchesList's patches on every input (see caelo_extract) */
#define CAELO_ST_TIES_LEFT 64     /* CAELO_EXTRACT_EXACT_PATCHES only: a kd-tree build gave up on its pass budget and a tie-split patch was
                                   * left on the canonical rule (flags & 2 still set) */
#define CAELO_EXTRACT_GIVEN_KEYPTS 8 /* caelo_extract / caelo_frame_job.mode bit: the CALLER's key points instead of the detector's (key point
                                        sources other than GetKeyPtsByAE, PoseEstimation.py:26-45): on entry key_pts rows [0, K) hold them
                                        (f32 xyz; in the pipeline rows[:, 60:63]) and *n_key = K in [1, 1024].  The ring image, response and
                                        key point kernels are skipped; one kernel checks K and the coordinates, writes valid (1.0 below K, 0.0
                                        from K on) and sets key_pixels to -1.  Voxel map, patches (CAELO_EXTRACT_EXACT_PATCHES included),
                                        dedup and encoder run as usual; rows below K keep the caller's xyz bits.  No CAELO_ST_FEW_KEYPTS: the
                                        reference asserts K > 50 only inside its own detector (SphericalRing.py:286) */
#define CAELO_EXTRACT_GIVEN_ROWS 16  /* caelo_frame_job.mode bit only (isLoadFeaturesFromFile, PoseEstimation.py:49-66): rows [1024][64]
                                        (descriptor zero-padded to columns 0:60 | xyz 60:63 | valid 63) and *n_key in [1, 1024] are INPUTS;
                                        pc may be NULL.  The batch runs no front and no encoder work, only the pair stage; key_pixels, flags
                                        and status are not written.  Zero padding leaves the float64 descriptor distances -- and so the
                                        match's certified argmin -- unchanged: 32-d descriptors (3DFeatNet) are matched the same way */
#define CAELO_ST_BAD_KEYPTS 128   /* CAELO_EXTRACT_GIVEN_KEYPTS only: K outside [1, 1024] (n_key is then set to 0), or a coordinate of a row
                                   * below K that is not finite or whose magnitude exceeds CAELO_GIVEN_KEYPTS_RANGE.  A deviation: the
                                   * reference raises nothing there (int32(nan) is INT_MIN and gives an empty patch) */
#define CAELO_GIVEN_KEYPTS_RANGE 16384.0 /* metres: the accepted |x|, |y|, |z| of a given key point.  Within it every key voxel and patch brick
                                          * index fits the 20-bit packing of the voxel tables (no aliasing), so a point off the scan or off
                                          * the voxel grid -- negative side included -- gets exactly the reference's patch (empty far away) */

#define CAELO_EXTRACT_CORRECT_PC 32   /* caelo_extract / caelo_frame_job.mode bit: the scan is first rotated by the context's calibration angle
                                        (caelo_set_calib_angle; CorrectPC, Transformations.py:28-39) into storage the library owns -- the voxel
                                        map's (caelo_extract) or the frame slot's (pipeline), max_points x 16 B, allocated by the first call in
                                        this mode -- and ring image and voxel map are built from that copy: the results of
                                        caelo_correct_pc + the same call without the bit, bit for bit.  The caller's pc is never written.  In the
                                        pipeline: one launch per batch at the head of the front stage.  A point on the z axis becomes NaN, as in
                                        the Python reference, and the frame reports CAELO_ST_NONFINITE.  Not with CAELO_EXTRACT_GIVEN_ROWS */

typedef struct caelo_ctx caelo_ctx;
typedef struct caelo_voxmap caelo_voxmap;

int caelo_abi_version(void);
/* How this binary was compiled (no reference counterpart; stamped by csrc/Makefile).  caelo/_ffi.py refuses to load a
 * library whose word has CAELO_BUILD_PACKED_F32 set: packed-f32 VALU instructions mis-execute in lanes 48-63 on MI355X
 * when three hardware queues are busy, so such a binary is silently wrong about once in 1 000 frames. */
#define CAELO_BUILD_PACKED_F32 1 /* built WITH v_pk_*_f32 (make PACKED_F32=1: the fault demonstrator, never the product) */
#define CAELO_BUILD_PROF 2       /* built with the per-phase cycle counters of the encoder (make PROF=1) */
#define CAELO_BUILD_STAMPED 256  /* the Makefile passed its flag word (a hand-rolled hipcc line that did not is refused too) */
int caelo_build_flags(void);
const char *caelo_last_error(void);
int caelo_create(caelo_ctx **ctx, int device);
void caelo_destroy(caelo_ctx *ctx);
/* Hardware self-check of the pose kernels (no reference counterpart): every lane of a wavefront derives the same RANSAC
 * hypothesis, so lanes that disagree mean a mis-executed instruction.  Synchronises the device and returns how many
 * wavefronts saw that since caelo_create.  0 on healthy hardware; tests and bench.py assert it. */
int caelo_lane_faults(caelo_ctx *ctx, int64_t *count_host);

/* Weights (HOST pointers, Keras layouts as stored in the .h5).  Replaces
 * keras.models.load_model(...) at Match.py:313,324 / Dirs.py:29-30. */
int caelo_set_respond_weights(caelo_ctx *ctx, const float *w1_host /*[3][3][3][32]*/, const float *b1_host /*[32]*/,
                              const float *w2_host /*[32][8]*/, const float *b2_host /*[8]*/);
int caelo_set_encoder_weights(caelo_ctx *ctx, const float *w1_host /*[27][1][8]*/, const float *b1_host,
                              const float *w2_host /*[27][8][16]*/, const float *b2_host,
                              const float *w3_host /*[27][16][32]*/, const float *b3_host,
                              const float *wd1_host /*[2048][200]*/, const float *bd1_host,
                              const float *wd2_host /*[200][20]*/, const float *bd2_host);
/* The encoder's activations.  The reference produces two sets: the shipped EncoderModel4VoxelPatch.h5 is tanh on all five layers,
 * its training script (AE4VoxelPatch.py:177-197) builds relu on the four hidden layers and a linear 20-d code.  hidden in
 * {CAELO_ACT_TANH, CAELO_ACT_RELU} is applied to conv3d_1..3 and dense_1 alike, code in {CAELO_ACT_TANH, CAELO_ACT_LINEAR} to dense_2;
 * anything else is CAELO_ERR_ARG.  A context starts as tanh / tanh.
 * caelo_set_encoder_model: weights and activations together; every derived operand image is rebuilt.  Refused (CAELO_ERR_ARG, the
 *   layer named in caelo_last_error, the context unchanged) when caelo_host_encoder_range finds a tensor the kernels split into f16
 *   halves that can leave the f16 range.
 * caelo_set_encoder_weights: these weights with the context's CURRENT activations.
 * caelo_host_encoder_range (host only, no device): worst-case magnitude of each layer's output in float64 over binary patches,
 *   kept per channel: b_1[c] = sum |w1[.][c]| + |b1[c]|, b_l[c] = sum_k |w_l[k][c]| b_(l-1)[channel of k] + |b_l[c]|, 1 behind a tanh layer;
 *   out[l-1] = max_c b_l[c].  Returns 0 when
 *   every split tensor fits (a tanh hidden stack always does), the 1-based number of the first layer whose output can exceed
 *   65504 where a kernel splits it -- layers 1..3 feed conv2, conv3 and Dense(200) as f16 halves; the hidden vector and the code
 *   stay f32 -- or CAELO_ERR_ARG.  The 32^3 entry points (caelo_patches32, caelo_encode32*) are tanh / tanh only and refuse any
 *   other model before launching. */
#define CAELO_ACT_TANH 0
#define CAELO_ACT_RELU 1
#define CAELO_ACT_LINEAR 2
int caelo_set_encoder_model(caelo_ctx *ctx, const float *w1_host, const float *b1_host, const float *w2_host, const float *b2_host,
                            const float *w3_host, const float *b3_host, const float *wd1_host, const float *bd1_host,
                            const float *wd2_host, const float *bd2_host, int hidden, int code);
int caelo_get_encoder_activations(caelo_ctx *ctx, int32_t out[2] /* hidden, code */);
int caelo_host_encoder_range(const float *w1_host, const float *b1_host, const float *w2_host, const float *b2_host,
                             const float *w3_host, const float *b3_host, const float *wd1_host, const float *bd1_host,
                             const float *wd2_host, const float *bd2_host, int hidden, int code, double out_host[5]);
/* on != 0: this context's encoder runs conv1 / conv2 with the exact-f32 kernel of round 2 instead of the default (f32 products
 * from 2-way f16 splits on the f16 matrix pipe) -- the precision reference of the tests and of tools/enc_layer_errors.py; slower.
 * An explicit, per-context choice: the library reads NO environment variable that changes arithmetic (no reference counterpart:
 * PatchEncoder.predict, Match.py:131-133, has one arithmetic). */
int caelo_set_encoder_reference(caelo_ctx *ctx, int on);

/* The decoder half of an autoencoder file (AE4VoxelPatch.py:199-211): Dense(200), Dense(2048), Reshape(4,4,4,32), Conv3D(16),
 * UpSampling3D(2), Conv3D(8), UpSampling3D(2), Conv3D(1).  hidden in {CAELO_ACT_TANH, CAELO_ACT_RELU} on the four hidden layers,
 * out = CAELO_ACT_SIGMOID; anything else is CAELO_ERR_ARG.  Host pointers, Keras layouts.  A context has no decoder until one is
 * set, and everything else behaves the same with or without one.  All arithmetic is f32 (f32-input matrix instructions), so there
 * is no range guard.
 * caelo_host_decoder_fold (host only, no device): UpSampling3D(2) + a 3^3 `same` convolution as eight parity classes of 2^3 taps on
 *   the source grid -- folded[p][o] = the sum, in float64 rounded once, of the taps t with ((p + t - 1) >> 1) - (p - 1) == o per axis
 *   (p, o, t as x*4+y*2+z resp. x*9+y*3+z); output voxel 2s + p reads source cell s + o + p - 1.
 * caelo_decode: codes[(p / group) * ld + (p % group) * 20 + j] f32 (group = 1, ld = 20: plain rows; group = 3, ld = 64: the
 *   pipeline's resident descriptor rows) -> any of prob [n][4096] f32 (x, y, z order: autoencoder.predict, AE4VoxelPatch.py:256),
 *   rebuilt [n][64] u64 (the packed patch layout; voxel set <=> (double)prob > threshold, Voxel.VoxelModel2PC's test),
 *   loss [n] f32 (Keras binary_crossentropy against target_bits [n][64]: mean over the 4096 voxels of -(y log p^ + (1 - y) log(1 - p^)),
 *   p^ = clip(p, 1e-7, 1 - 1e-7)) and counts [n][3] i32 (voxels set in the target, in rebuilt, in both; the first and the last are 0
 *   without a target).  Every output may be NULL, not all of them.  CAELO_ERR_ARG before any launch: no decoder set, loss without
 *   target, threshold outside (0, 1) or not finite, group * 20 > ld, n < 0, no output.  n = 0 does nothing.  ws: caelo_decode_ws_bytes(n)
 *   bytes, no initialisation needed, one per stream.  A patch's outputs do not depend on n or on its position.
 * caelo_decode_ws_layout (test aid): out[0] = byte offset in ws of G4 [n][2048] f32 (Dense(2048)'s activated output), out[1] = its rows. */
#define CAELO_ACT_SIGMOID 3
int caelo_set_decoder_model(caelo_ctx *ctx, const float *wd3_host /*[20][200]*/, const float *bd3_host, const float *wd4_host /*[200][2048]*/,
                            const float *bd4_host, const float *w4_host /*[27][32][16]*/, const float *b4_host,
                            const float *w5_host /*[27][16][8]*/, const float *b5_host, const float *w6_host /*[27][8][1]*/,
                            const float *b6_host, int hidden, int out);
int caelo_get_decoder_activations(caelo_ctx *ctx, int32_t out[2] /* hidden, out */);
int caelo_host_decoder_fold(const float *w /*[27][cin][cout]*/, int cin, int cout, float *folded /*[8][8][cin][cout]*/);
int64_t caelo_decode_ws_bytes(int64_t n_patches);
int caelo_decode_ws_layout(int64_t n_patches, int64_t out[2]);
int caelo_decode(caelo_ctx *ctx, const float *codes, int64_t n_patches, int group, int ld, const uint64_t *target_bits, double threshold,
                 float *prob, uint64_t *rebuilt, float *loss, int32_t *counts, void *ws, void *stream);

/* Training the voxel-patch autoencoder (AE4VoxelPatch.py:186-213): loss and gradient of the whole network, and Keras 2.3's Adadelta.
 * The weights are plain Keras-layout f32 in ONE flat device buffer of 864 741 floats: the 20 tensors conv3d_1 .. dense_2, dense_3 ..
 * conv3d_6, kernel then bias per layer (caelo_train_param_layout: out[t] = {offset, count} in floats).  Nothing here reads or
 * changes the context's inference models.  f32 operands and accumulation (f32-input matrix instructions), no floating-point atomics.
 * caelo_autoencoder_grad: bits [n][64] u64 (the packed patch layout) -> loss[0] (device f32) = the mean over patches of the mean over
 *   the 4096 voxels of Keras's binary_crossentropy (caelo_decode's loss), and grads = dloss / dparams in params' layout (NULL: forward
 *   only; the loss bits are those of the full call).  enc_hidden / dec_hidden in {CAELO_ACT_TANH, CAELO_ACT_RELU}, enc_code in
 *   {CAELO_ACT_TANH, CAELO_ACT_LINEAR}.  relu' = (y > 0), tanh' = 1 - y^2 from the stored output; a pooling window's gradient goes to
 *   its first maximum in ascending (dx, dy, dz) order, dz fastest; dloss/dz = (sigmoid(z) - y) / (4096 n) where |z| <= logit(1 - 1e-7),
 *   0 beyond.  The batch is walked in chunks of `chunk` patches, whose partial gradients are added in ascending order: the same
 *   (n, chunk) gives the same bits in every call; the loss bits depend on n alone.  ws: caelo_train_ws_bytes(chunk) bytes, no
 *   initialisation needed, one per stream.  CAELO_ERR_ARG before any launch: n < 0, chunk outside [1, 8192], a null pointer, an
 *   activation code outside the sets above.  n = 0 writes loss 0 and zero gradients.
 * caelo_train_ws_layout (test aid): byte offsets in ws of what the LAST chunk left -- out[0] dloss/dz [chunk][4096], out[1]
 *   dloss/dcode [chunk][20] (the activated code), out[2] dloss/dP1 [chunk][8^3 x 8] (the first pooling's output).
 * caelo_adadelta_step: a = rho a + (1 - rho) g^2; u = g sqrt(d + eps) / sqrt(a + eps); p -= lr u; d = rho d + (1 - rho) u^2 over
 *   `count` floats, every operation rounded on its own in f32, sqrt and the quotient correctly rounded (Keras 2.3's defaults: lr 1,
 *   rho 0.95, eps 1e-7). */
int caelo_train_param_layout(int64_t out[20][2]);
int64_t caelo_train_ws_bytes(int64_t chunk);
int caelo_train_ws_layout(int64_t chunk, int64_t out[3]);
int caelo_autoencoder_grad(caelo_ctx *ctx, const float *params, int enc_hidden, int enc_code, int dec_hidden, const uint64_t *bits, int64_t n,
                           int64_t chunk, float *grads, float *loss, void *ws, void *stream);
int caelo_adadelta_step(caelo_ctx *ctx, float *params, const float *grads, float *acc_g, float *acc_d, int64_t count, float lr, float rho,
                        float eps, void *stream);

/* Training the spherical-ring autoencoder (AE4SphericalRingPC.py:129-144), whose conv2d_1 / conv2d_2 are the response layer: loss and
 * gradient of the whole network, and Keras 2.2.4's Adam.  Input [n][h][w][3] -> conv2d_1 3x3 3->32 relu, conv2d_2 1x1 32->8 relu,
 * MaxPooling2D(2), conv2d_3 3x3 8->16 relu, MaxPooling2D(2), conv2d_4 3x3 16->16 relu, UpSampling2D(2), conv2d_5 3x3 16->8 relu,
 * UpSampling2D(2), conv2d_6 1x1 8->3 linear; loss = mean_squared_error against the input.  The weights are plain Keras-layout f32 in
 * ONE flat device buffer of 5 835 floats: 12 tensors, kernel then bias per layer (caelo_ring_train_param_layout: out[t] = {offset,
 * count} in floats).  Nothing here reads or changes the context's inference models.  f32 operands and accumulation (f32-input matrix
 * instructions), no floating-point atomics.
 * caelo_ring_autoencoder_grad: pixel (i, y, x) channel c (0..2) is images[i img_stride + y row_stride + x pix_stride + c], strides in
 *   floats, so a batch of projected rings [n][69][1800][5] is read in place at h = 64, w = 1792 (caelo_respond's in_w / in_c idea).
 *   loss[0] (device f32) = the mean of (r - x)^2 over all 3 n h w elements, summed in double in a fixed tree and rounded once; grads =
 *   dloss / dparams in params' layout (NULL: forward only; the loss bits are those of the full call); recon (optional) [n][h][w][3] =
 *   autoencoder.predict.  relu' = (y > 0) from the stored output; a pooling window's gradient goes to its first maximum in ascending
 *   (dy, dx) order, dx fastest (torch's max_pool2d rule; TensorFlow's is unpinned); UpSampling2D's adjoint sums the four children in
 *   that order.  The batch is walked in chunks of `chunk` images whose partial weight gradients are added in ascending order: the same
 *   (n, h, w, chunk) gives the same bits in every call; the loss bits depend on (n, h, w) alone.  ws: caelo_ring_train_ws_bytes(h, w,
 *   chunk) bytes (0 for a shape that is refused), no initialisation needed, one per stream.  CAELO_ERR_ARG before any launch: n < 0; h
 *   or w not a positive multiple of 4 (Keras would pad its 'same' poolings there; not built) or h w > 2^24; strides that make pixels
 *   overlap (pix_stride < 3, row_stride < w pix_stride, img_stride < h row_stride); chunk outside [1, 4096]; a null params, loss, ws,
 *   or images with n > 0.  n = 0 writes loss 0 and zero gradients.
 * caelo_ring_train_ws_layout (test aid): byte offsets in ws of what the LAST chunk left -- out[0] A2 [chunk][h][w][8] (the response
 *   layer's activated output), out[1] r [chunk][h][w][3], out[2] dloss/dP1 [chunk][h/2][w/2][8], out[3] dloss/dr [chunk][h][w][3].
 * caelo_adam_step: m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; p -= (lr_t m) / (sqrt(v) + eps) over `count` floats,
 *   every operation rounded on its own in f32, sqrt and the quotient correctly rounded, no fused multiply-add.  lr_t = lr sqrt(1 -
 *   beta2^t) / (1 - beta1^t) is the CALLER's, computed in float64 and rounded to f32 once (TensorFlow's f32 pow cannot be pinned).
 *   Keras's eps sits OUTSIDE the bias correction: torch.optim.Adam divides by sqrt(v / (1 - beta2^t)) + eps instead, a different
 *   update, so it is not the yardstick.  Keras 2.2.4's defaults: lr 0.001, beta1 0.9, beta2 0.999, eps 1e-7. */
int caelo_ring_train_param_layout(int64_t out[12][2]);
int64_t caelo_ring_train_ws_bytes(int h, int w, int64_t chunk);
int caelo_ring_train_ws_layout(int h, int w, int64_t chunk, int64_t out[4]);
int caelo_ring_autoencoder_grad(caelo_ctx *ctx, const float *params, const float *images, int64_t n, int h, int w, int64_t img_stride,
                                int64_t row_stride, int64_t pix_stride, int64_t chunk, float *grads, float *loss, float *recon, void *ws,
                                void *stream);
int caelo_adam_step(caelo_ctx *ctx, float *params, const float *grads, float *m, float *v, int64_t count, float lr_t, float beta1, float beta2,
                    float eps, void *stream);

/* CorrectPC  (Transformations.py:28-39; BatchPreprocess.py:70-88 BatchCorrectPC): every point rotated by calib_angle_deg about the
 * axis p x z^, the HDL-64E's vertical-angle calibration of the KITTI scans.  pc, out [n][stride] f32 (device), stride 3 or 4; with
 * stride 4 the fourth column (intensity) is copied bit for bit.  out may not overlap pc; n = 0 does nothing; a non-finite angle is
 * refused.  Arithmetic: the reference's float32 operations under NumPy >= 2 (NEP 50) one by one up to the rotation matrix (its
 * bits); the final product is p'_i = (R_i0 x + R_i1 y) + R_i2 z without contraction, where the reference calls its BLAS (DESIGN.md
 * 5.8).  A point with x = y = 0 gives NaN, as there.
 * caelo_set_calib_angle: the angle (degrees, finite; 0 until set) that CAELO_EXTRACT_CORRECT_PC applies -- a context setting like
 * the weights, read when a call or a pipeline batch is launched. */
int caelo_correct_pc(caelo_ctx *ctx, const float *pc, int64_t n, int stride, double calib_angle_deg, float *out, void *stream);
int caelo_set_calib_angle(caelo_ctx *ctx, double deg);
double caelo_get_calib_angle(caelo_ctx *ctx);

/* ProjectPC2SphericalRing  (SphericalRing.py:72-94)
 * pc [n][4] f32 -> ring [69][1800][5] f32, counter [69][1800] i32.  workspace: winner [69*1800] i32. */
int caelo_project(caelo_ctx *ctx, const float *pc, int64_t n, float *ring, int32_t *counter, int32_t *winner_ws,
                  int32_t *status, void *stream);

/* RespondLayer.predict  (SphericalRing.py:405-408; SphericalRingPCRespondLayer.h5)
 * in [rows>=64][in_w][in_c] (channels 0..2 of rows 0..63, cols 0..1791) -> resp [64][1792][8] */
int caelo_respond(caelo_ctx *ctx, const float *in, int in_w, int in_c, float *resp, void *stream);

/* GetKeyPtsByAE  (SphericalRing.py:113-291).  ring_c = 5: demo mode (:414); 3: batch mode
 * (BatchPreprocess.py:97-98,131-136).  workspace: ws of caelo_keypoints_ws_bytes() bytes, 16-byte aligned.
 * outputs: key_pixels [1024][2] i64 (row,col), key_pts [1024][3] f32, n_key [1] i32. */
int64_t caelo_keypoints_ws_bytes(void);
int caelo_keypoints(caelo_ctx *ctx, const float *ring, int ring_w, int ring_c, const int32_t *counter, int cnt_w,
                    const float *resp, void *ws, int64_t *key_pixels, float *key_pts, int32_t *n_key,
                    int32_t *status, void *stream);

/* debug aid: out_host[40] = 16 phase timestamps (100 MHz ticks) of the last keypoint-selection kernel, 16 of the
 * last encoder stage-1 kernel (workgroup 0, first patch), 8 of the last patch-gather kernel */
int caelo_debug_read(unsigned long long *out_host);

/* Voxelization  (Voxel.py:100-173) into a device voxel map (3 scales of 8^3-voxel bricks). */
int caelo_voxmap_create(caelo_ctx *ctx, int64_t max_points, caelo_voxmap **map);
void caelo_voxmap_destroy(caelo_voxmap *map);
int caelo_voxelize(caelo_ctx *ctx, caelo_voxmap *map, const float *pc, int64_t n, int stride, int32_t *status,
                   void *stream);
/* The one-pass build caelo_extract uses (scales 1/2 derived from the scale-0 bricks, points within an ulp of a voxel
 * face resolved through their voxel's first point): same voxel SETS as caelo_voxelize, no first-touch order, so
 * caelo_voxmap_export does not apply; caelo_patches and caelo_voxmap_dump do. */
int caelo_voxelize_fast(caelo_ctx *ctx, caelo_voxmap *map, const float *pc, int64_t n, int stride, int32_t *status,
                        void *stream);
/* Occupied 8x8x8-voxel bricks of one scale, unordered: keys [capacity] u64 (brick x << 40 | y << 20 | z),
 * bits [capacity][8] u64 (word = x & 7, bit = (y & 7) * 8 + (z & 7)), count [1] i32 (device, may exceed capacity:
 * then only `capacity` bricks were written).  Diagnostic / test access to the device voxel map. */
int caelo_voxmap_dump(caelo_ctx *ctx, const caelo_voxmap *map, int scale, uint64_t *keys, uint64_t *bits, int64_t capacity,
                      int32_t *count, void *stream);
/* The map's build counters, counts8 [8] i32 (device): [0..2] voxels of scales 0, 1, 2 (what the 496-voxel check reads); after a
 * one-pass build also [4] entries of the scale-0 brick list (holes included), [5] scale-1 bricks listed, [6] points within an
 * ulp of a voxel face.  Diagnostic / test access. */
int caelo_voxmap_counts(caelo_ctx *ctx, const caelo_voxmap *map, int32_t *counts8, void *stream);
/* AllVoxels0/1/2 in the reference's order (first touch; scale 0 block-grouped, Voxel.py:161-165).
 * out [capacity][3] i16 per scale, counts [3] i64 (device).  Valid after caelo_voxelize.  Asynchronous on `stream`: a count
 * above `capacity` means only the first `capacity` voxels of that scale were written (the caller checks after reading counts). */
int caelo_voxmap_export(caelo_ctx *ctx, caelo_voxmap *map, int16_t *all0, int16_t *all1, int16_t *all2,
                        int64_t capacity, int64_t *counts, void *stream);
/* Records the first-touch order of the map's voxel lists (scales in `scale_mask`, bit s = scale s) on the device, so that
 * caelo_patches on THIS map redoes its tie-split patches in scikit-learn's kd-tree order (csrc/kdorder.hip) -- what
 * caelo_voxmap_export + caelo_voxmap_from_lists + caelo_patches give, without the lists leaving the map and without a host
 * round trip for their lengths.  Valid after caelo_voxelize (which records first touch); asynchronous on `stream`.  A tie-split
 * patch of a scale outside the mask keeps the canonical rule and flag bit 2. */
int caelo_voxmap_order(caelo_ctx *ctx, caelo_voxmap *map, int scale_mask, void *stream);
/* Build the map from reference-format lists instead (GetPatchesList called with arrays). */
int caelo_voxmap_from_lists(caelo_ctx *ctx, caelo_voxmap *map, const int16_t *all0, int64_t n0, const int16_t *all1,
                            int64_t n1, const int16_t *all2, int64_t n2, int32_t *status, void *stream);

/* GetPatchesList  (Voxel.py:177-216): pts [k][3] f32 (k read from n_key when non-null, else k_max)
 * -> bits [k_max][3][64] u64, flags [k_max][3] u8 (bit0 truncated by the 496-NN cap; bit1 the cut falls inside a class of
 * equidistant voxels and the patch is on the canonical rule -- the map has no ordered lists, or the kd build gave up; bit2 such a
 * patch redone in the library's own order: scikit-learn's kd-tree from 994 voxels on, np.argpartition's below (csrc/kdorder.hip)). */
int caelo_patches(caelo_ctx *ctx, const caelo_voxmap *map, const float *pts, int64_t k_max, const int32_t *n_key,
                  uint64_t *bits, uint8_t *flags, int32_t *status, void *stream);
/* The same for n <= 8 maps / key point sets (arrays of n HOST pointers to the device buffers of caelo_patches): the gathers one after the
 * other, then the kd-tree redo of the tie-split patches of ALL of them behind one launch of each kd kernel -- the chain of a redo (a
 * millisecond or two of dependent quickselect passes, Voxel.py:195-196 in scikit-learn's order) is paid once per set, not per frame. */
int caelo_patches_many(caelo_ctx *ctx, int n, const caelo_voxmap *const *maps, const float *const *pts, int64_t k_max,
                       const int32_t *const *n_key, uint64_t *const *bits, uint8_t *const *flags, int32_t *const *status, void *stream);
/* The kd-tree of one scale as the last caelo_patches / caelo_patches_many on this map left it (csrc/kdorder.hip), read back into
 * HOST buffers; waits for `stream`.  Diagnostic / test access, no hot path touches it (additive; the ABI version stays 6).
 *   state [32] i32   the map's kd words: [0..2] tie-split patches queued per scale | [4..6] 0 no tree, 1 built, 2 not built (the build
 *                    gave up on its work budget, or too many nodes: the canonical rule stays) | [16..18] list lengths
 *   idx [n] i32      the tree's index array (positions in the list)          start, end [n_nodes] i32   node i owns idx[start, end)
 *   lo, hi [n_nodes][3] i16   bounding boxes                                 counts [3] i64 = n, n_nodes (2^n_levels - 1; 0 below 994),
 *                    the number of upper levels the build runs in one workgroup before each subtree gets its own
 * What idx and the node tables hold is meaningful only where state[4 + scale] == 1.  CAELO_ERR_ARG for a map without ordered lists
 * (caelo_voxmap_from_lists, caelo_voxmap_order), CAELO_ERR_CAPACITY when n > idx_capacity or n_nodes > node_capacity (counts is
 * written, nothing else is copied). */
int caelo_voxmap_kd_dump(caelo_ctx *ctx, const caelo_voxmap *map, int scale, int32_t *state, int32_t *idx, int64_t idx_capacity,
                         int32_t *start, int32_t *end, int16_t *lo, int16_t *hi, int64_t node_capacity, int64_t *counts, void *stream);
/* dense <-> packed conversion for callers that want the reference's [K,16,16,16,1] f32 arrays */
int caelo_unpack_patches(caelo_ctx *ctx, const uint64_t *bits, int64_t n_patches, float *dense, void *stream);
int caelo_pack_patches(caelo_ctx *ctx, const float *dense, int64_t n_patches, uint64_t *bits, void *stream);

/* PatchEncoder.predict / GetFeaturesFromPatches  (Match.py:130-135; EncoderModel4VoxelPatch.h5)
 * bits [n_patches][64] u64 -> out[(p / group) * out_stride + (p % group) * 20 + j].
 * group = 1, out_stride = 20: plain predict; group = 3, out_stride = 60 on [K][3][64]: Features [K][60].
 * workspace: ws of caelo_encode_ws_bytes(n_patches) bytes, zero-filled ONCE by its owner before the first call
 * (its header holds work counters that every call returns to zero), one ws per stream.
 * caelo_encode_ws_layout (test aid): byte offsets in ws of what the four kernels leave behind -- out[0] P2 [np][1024] f32 (after
 * pool2), out[1] F3 [np][2048] (after conv3), out[2] Dense(200) partial sums [slices][np][208]; out[3] = np (rows padded to whole
 * row tiles), out[4] = k slices in use, out[5] = k slices the buffer is sized for. */
int64_t caelo_encode_ws_bytes(int64_t n_patches);
int caelo_encode_ws_layout(int64_t n_patches, int64_t out[6]);
int caelo_encode(caelo_ctx *ctx, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                 void *ws, void *stream);

/* ---- BASELINE.json configs[4]: 32^3 patches (a stress case of this repo, NOT a reference code path) ----------
 * The reference has PatchSize = 16 only (Voxel.py:31-33).  These three entry points keep GetPatchesList's rule
 * (Voxel.py:177-216: key voxel in f64, wrap-around placement) with the window [-16,16)^3 and the 496-NN cap
 * disabled, and the encoder's layer stack (Match.py:130-135) on 32^3 inputs: Flatten is 16384 wide, so dense_1
 * is a caller-supplied [16384][200] matrix (host pointers, like caelo_set_encoder_weights; conv kernels, biases
 * and dense_2 are the ones already set).
 * bits [k_max][3][512] u64: voxel (ix,iy,iz) at bit (lin & 63) of word (lin >> 6), lin = (ix*32 + iy)*32 + iz.
 * caelo_encode32: bits [n_patches][512] -> out[(p / group) * out_stride + (p % group) * 20 + j]; ws of
 * caelo_encode32_ws_bytes(n_patches) bytes (no initialisation needed).
 * caelo_encode32_ws_layout (test aid): byte offsets in ws of what the kernels leave behind -- out[0] P1 [n_patches][16^3][8] f32
 * (after conv1 + pool), out[1] P2 [n_patches][8^3][16] (after conv2 + pool), out[2] F3 [np][16384] (after conv3), out[3] Dense(200)
 * partial sums [slices][np][208]; out[4] = np (rows padded to whole row tiles), out[5] = k slices in use, out[6] = k slices the
 * buffer is sized for. */
int caelo_patches32(caelo_ctx *ctx, const caelo_voxmap *map, const float *pts, int pts_ld, int64_t k_max,
                    const int32_t *n_key, uint64_t *bits, void *stream);
int caelo_set_encoder32_dense(caelo_ctx *ctx, const float *wd1, const float *bd1);
int64_t caelo_encode32_ws_bytes(int64_t n_patches);
int caelo_encode32_ws_layout(int64_t n_patches, int64_t out[7]);
int caelo_encode32(caelo_ctx *ctx, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                   void *ws, void *stream);

/* caelo_encode32 with a HIP event between its launches; synchronises; ms_host[4] = conv1+pool, conv2+pool, conv3,
 * Dense(200)+head in ms (measurement aid for bench.py --config 5) */
int caelo_encode32_profile(caelo_ctx *ctx, const uint64_t *bits, int64_t n_patches, int group, float *out, int out_stride,
                           void *ws, void *stream, float *ms_host);

/* caelo_encode with a HIP event between its four kernels (stage1 = conv1+pool1+conv2+pool2, conv3,
 * dense1, head) on the launch stream; synchronises, writes the durations in ms to ms_host[0..3] and the number of
 * MFMA instructions stage 1 actually executed, in millions, to ms_host[4] (it skips all-background rows) and the FLOPs of
 * one such instruction to ms_host[5] (16384: v_mfma_f32_16x16x32_f16; 2048: the f32-input kernel).  ms_host holds 6 floats. */
int caelo_encode_profile(caelo_ctx *ctx, const uint64_t *bits, int64_t n_patches, int group, float *out,
                         int out_stride, void *ws, void *stream, float *ms_host);

/* NN match  (Match.py:257-258): pair_idx[j] = argmin_i ||f0[i]-f1[j]|| (f64, first minimum).
 * f0 [k0][ld0], f1 [k1][ld1] (leading dimensions in floats, >= dim, dim <= 256; wider: CAELO_ERR_ARG); k0/k1 read from the
 * n0/n1 device words when non-null.
 * ws: a call with dim <= 64 is sized by caelo_match_ws_bytes(max(k0_max, k1_max)), a call with dim > 64 by
 * caelo_match_ws_bytes_dim(max(k0_max, k1_max), dim) (which returns caelo_match_ws_bytes' figure for dim <= 64 and never
 * shrinks as dim grows: a workspace sized for the widest descriptor serves every call): two statistics counters the calls only add to (columns re-scanned
 * exactly, columns decided between two rows; zero-fill the first 256 bytes once if you read them) and the scratch images of
 * the two frames (every call rewrites them).  Nothing crosses workgroups.  The distances are screened on the f16 matrix pipe
 * inside a rigorous error window and only the rows that can be the minimum are evaluated in float64 like scipy's cdist: the
 * result is the float64 argmin, bit for bit. */
int64_t caelo_match_ws_bytes(int64_t k_max);
int64_t caelo_match_ws_bytes_dim(int64_t k_max, int dim);
int caelo_match(caelo_ctx *ctx, const float *f0, int ld0, int64_t k0_max, const int32_t *n0, const float *f1, int ld1,
                int64_t k1_max, const int32_t *n1, int dim, int64_t *pair_idx, void *ws, void *stream);

/* Measurement aid (no reference counterpart): the pipeline's launch shape of the NN match -- n_pairs (<= 8) pairs of consecutive
 * frame rows (rows [n_pairs + 1] device pointers to [1024][64] f32, descriptor in columns 0:60; n_key [n_pairs + 1] device counts
 * or NULL) behind one k_match_prep + one k_match_screen launch, `repeats` times between HIP events on `stream`.
 * pair_idx [n_pairs][1024] out; ws: n_pairs * caelo_match_ws_bytes(1024) bytes; ms_host[2] = both kernels / the prep alone, averaged. */
int caelo_match_profile(caelo_ctx *ctx, const float *const *rows, int n_pairs, const int32_t *const *n_key, int64_t *pair_idx,
                        void *ws, int repeats, void *stream, float *ms_host);

/* SolveRT  (Match.py:138-158): p0 ~ R p1 + T over n point pairs.  R [9], T [3] f32 (device);
 * credible [1] i32 (optional): the reference's isCredible, -1 when det(R) < 0 was met. */
int caelo_solve_rt(caelo_ctx *ctx, const float *p0, const float *p1, int64_t n, float *R, float *T,
                   int32_t *credible, void *stream);

/* RANSAC4RT + SolveRelativePose tail  (Match.py:162-218, :260-283).
 * pc0 [k0][ld0], pc1 [k1][ld1] (xyz in the first 3 columns), pair_idx [k1]; rand [3*500][4] f64 = the uniform doubles the
 * reference's np.random.random((4,)) would return, in consumption order.
 * result (device, caelo_pose_result) + inlier mask [k1_max] u8 (4-byte aligned for dword stores).  workspace ws:
 * caelo_ransac_ws_bytes() bytes (the hypotheses' inlier counts between the two kernels of a call; no
 * initialisation), one ws per call in flight. */
typedef struct {
    float R[9];           /* final refit rotation, row-major */
    float T[3];
    float R_ransac[9];    /* best hypothesis before the refit (RANSAC4RT's R_star) */
    float T_ransac[3];
    float threshold;      /* residualThreshold returned (0.4 / 0.8 / 1.6) */
    int32_t success;      /* isSuccess */
    int32_t iterations;   /* cntIters of the last level */
    int32_t n_inliers;
    int32_t best_trial;   /* index into rand of the winning hypothesis, -1 if none */
    int32_t n_pairs;
} caelo_pose_result;
/* The certificate a RANSAC call leaves for the host half (optional, device memory, 16-byte aligned): for each of the 500
 * hypotheses of the first threshold level an UPPER BOUND `hi` on the inlier count the reference's own arithmetic can give it --
 * NumPy forms the 4-point covariance, R, T and the residuals in float32 through its BLAS (Match.py:141-157,:190-193), so a
 * count depends on that BLAS's rounding; the kernels fit in float64 and count the pairs whose residual lies below the
 * threshold PLUS a bound on that difference -- the four sample indices of each hypothesis, and the matched pairs
 * (P0[pair_idx[i]], P1[i]).  caelo_host_certify replays Match.py:181-214 over the bounds and re-evaluates the deciding
 * hypotheses through NumPy's BLAS / LAPACK entry points: inlier sets, R_star / T_star and the refit are then the reference's
 * bits on this host. */
#define CAELO_CERT_MAX_PAIRS 1024
#define CAELO_CERT_MAGIC 0x43455254
#define CAELO_CERT_NO_BOUNDS 1    /* flags: more than CAELO_CERT_MAX_PAIRS pairs -- no bounds, no pairs stored */
typedef struct {
    int32_t magic;        /* CAELO_CERT_MAGIC once k_ransac_finish has written the record */
    int32_t n_pairs;      /* N */
    int32_t flags;
    int32_t levels_up;    /* 1: hi_up / idx_up hold the bounds of the 0.8 m and 1.6 m levels (written by the pipeline's kernels for a pair
                           * whose first level reached leastInliers with no hypothesis: Match.py:207-214) */
    int32_t reserved[12];
    int32_t hi[512];      /* [500] used */
    int32_t idx[512][4];  /* sample indices int32(u * N) (Match.py:182-184) of the first level's hypotheses */
    float p0[CAELO_CERT_MAX_PAIRS][3]; /* Pairs0 = PC0[pairIdx] (Match.py:260) */
    float p1[CAELO_CERT_MAX_PAIRS][3]; /* Pairs1 */
    int32_t hi_up[2][512];      /* the same for the hypotheses of the 0.8 m and the 1.6 m level (draws 500 .. 999, 1000 .. 1499) */
    int32_t idx_up[2][512][4];
} caelo_ransac_cert;
int64_t caelo_cert_bytes(void);
int64_t caelo_ransac_ws_bytes(void);
int caelo_ransac(caelo_ctx *ctx, const float *pc0, int ld0, const float *pc1, int ld1, const int64_t *pair_idx,
                 int64_t k1_max, const int32_t *n1, const double *rand, caelo_pose_result *result,
                 uint8_t *inlier_mask, void *ws, caelo_ransac_cert *cert, void *stream);

/* Host half of the exact RANSAC (csrc/certify.hip; every pointer below is HOST memory, no device is touched).
 * caelo_host_bind_blas: the cblas_sgemm / cblas_sgemv / dgesdd (Fortran) entry points of the BLAS the process's NumPy is
 *   linked against (caelo/hostblas.py finds them), ilp64 = 1 when their integers are 64 bits wide.  Process-wide.
 * caelo_host_solve_rt: SolveRT (Match.py:138-158) by NumPy's own call sequence -- float32 row sums, cblas_sgemm for the
 *   covariance, dgesdd on its float64 copy, U / Vh cast to float32, cblas_sgemm for R, cblas_sgemv for T.
 * caelo_host_ransac: RANSAC4RT + the refit of SolveRelativePose (Match.py:162-218,:269-283) on pairs [n][3]; with `hi`
 *   (the first level's bounds) only the deciding hypotheses are evaluated, without it all of them, like the reference.
 * caelo_host_certify: k certificates (copied from the device) -> k results + masks [k][mask_ld]; rand_host [k] (nullable, as
 *   may be its entries) = the pairs' draws, needed only when a pair escalates beyond 0.4 m; evals [k] (nullable) = hypotheses
 *   evaluated; status [k] (nullable): 0 exact, 1 the draws were needed and missing, 2 no bounds in the record (more than
 *   1024 pairs: use caelo_host_ransac), 3 no record.  `threads` host threads share the k records. */
int caelo_host_bind_blas(void *cblas_sgemm, void *cblas_sgemv, void *dgesdd, int ilp64);
int caelo_host_blas_bound(void);
int caelo_host_unbind_blas(void);   /* forget the bound entry points (a library that failed the binder's bit-for-bit check) */
/* one BLAS / LAPACK call of the host half, issued exactly as the host half issues it (flags, leading dimensions): what a binder
 * compares with np.dot / np.linalg.svd.  op 0: out[9] = a^T b, a, b [n][3]; 1: out[18] = U | Vh of svd(a [3][3]); 2: out[9] = a^T b^T,
 * [3][3] each; 3: out[3] = a b, a [3][3], b [3]; 4: out[3][n] = a b^T, a [3][3], b [n][3] */
int caelo_host_blas_probe(int op, const float *a_host, const float *b_host, int64_t n, float *out_host);
/* exact hypothesis counts the host half found ABOVE the device's upper bound since the process started.  The bound's constant is
 * calibrated, not proven: the host half checks every count it evaluates, and on a violation decides the pair by the reference's
 * loop without bounds (still exact) and counts it here.  0 on every run so far. */
int64_t caelo_host_bound_violations(void);
int caelo_host_solve_rt(const float *p0_host, const float *p1_host, int64_t n, float *R_host, float *T_host, int32_t *credible_host);
int caelo_host_ransac(const float *pairs0_host, const float *pairs1_host, int64_t n, const double *rand_host, const int32_t *hi_host,
                      caelo_pose_result *result_host, uint8_t *mask_host, int32_t *evals_host);
int caelo_host_certify(const void *certs_host, int64_t k, const double *const *rand_host, caelo_pose_result *results_host,
                       uint8_t *masks_host, int64_t mask_ld, int32_t *evals_host, int32_t *status_host, int threads);

/* Fused per-scan hot path: ProjectPC2SphericalRing -> RespondLayer.predict -> GetKeyPtsByAE ->
 * Voxelization -> GetPatchesList -> GetFeaturesFromPatches in one call, one stream, no host sync.
 * pc [n][4] f32.  dist_channels 5 = demo calling mode (SphericalRing.py:414), 3 = batch mode
 * (BatchPreprocess.py:97-98,131-136).  Outputs (device): key_pts rows [1024][kp_ld], features rows
 * [1024][feat_ld] (60 used), valid (optional) [1024] with stride valid_ld = 1.0 for rows < K,
 * key_pixels [1024][2], n_key [1], flags [1024][3] (caelo_patches), status int32[4] 16-byte aligned
 * (word 0 = CAELO_ST_* bits, cleared by the call).  ws: caelo_extract_ws_bytes() bytes, 256-byte aligned, zero-filled
 * once by its owner before the first call (it embeds an encoder workspace), one ws per stream.
 * mode: CAELO_EXTRACT_* bits.  By default the voxel maps are SETS: where the 496-nearest cut (Voxel.py:195-196) splits a class of
 * equidistant voxels the patch follows a canonical rule and carries flags & 2.  CAELO_EXTRACT_EXACT_PATCHES returns the reference's
 * patches instead, in the same call and with no host involvement: the two-pass first-touch voxelization (implies
 * CAELO_EXTRACT_EXACT_VOXELS), a device-side count of the tie-split patches per scale, the first-touch lists of only the (frame, scale)
 * pairs that hold one, and the redo of those patches before the encoder runs -- scikit-learn's kd-tree from 994 voxels on,
 * np.argpartition's introselect below (what caelo_voxelize + caelo_voxmap_order + caelo_patches + caelo_encode give).  Redone
 * patches carry flags & 4.  A kd build that gives up on its pass budget leaves its patches on the canonical rule (flags & 2) and
 * sets CAELO_ST_TIES_LEFT in the status word.  The first call in this mode allocates the map's kd storage (about
 * 3 x max_points x 30 B plus 3 x 16384 x 20 B of node tables) and its ordering scratch (about 12 B per first-touch table slot plus
 * 3 x max_points x 24 B of sort buffers); later calls allocate nothing.  Frames without a tie-split patch get the default mode's
 * results, bit for bit. */
int64_t caelo_extract_ws_bytes(void);
/* Byte offset, inside the caelo_extract workspace, of the frame buffer the last call left: the bit-packed patches [3072][64] u64 (patch
 * = key point * 3 + scale) followed by the de-duplication tables -- int32 count, 63 int32 of padding, int32 list[3072] (the patches
 * that were encoded, coarsest scale first), int32 slot_of[3072] (a listed patch: its position in list; a copy: -(representative + 1)).
 * Read-only; meant for tests of the de-duplication. */
int64_t caelo_extract_ws_frame_offset(void);
/* Byte offset, inside the caelo_extract workspace, of the key point eligibility map the last call left: 64 u64 words, one per ring row
 * 0..63; bit b of word y is set iff some pixel of columns 32 b .. 32 b + 31 of row y holds a point whose norm over the first
 * dist_channels ring channels is >= 10 (the range gate of SphericalRing.py:197-198).  Read-only; meant for tests. */
int64_t caelo_extract_ws_kp_eligible_offset(void);
int64_t caelo_extract_ws_ring_offset(void);   /* the fused path's ring image [69][1800][5] f32 (read-only, for tests) */
int caelo_extract(caelo_ctx *ctx, caelo_voxmap *map, const float *pc, int64_t n, int dist_channels, int mode, float *key_pts,
                  int kp_ld, float *features, int feat_ld, float *valid, int valid_ld, int64_t *key_pixels,
                  int32_t *n_key, uint8_t *flags, int32_t *status, void *ws, void *stream);

/* ExtendKeyPtsInShpericalRing  (SphericalRing.py:294-317; BatchPreprocess.py:139): the occupied ring pixels of the
 * 13 x 13 window of every keypixel, keypixels in order, each window row-major, a pixel only for the FIRST keypixel
 * whose window covers it.  Like the reference it ZEROES those windows in the caller's counter.
 * ring [>=rows][ring_w][ring_c] f32, counter [>=rows][cnt_w] i32 (in/out); rows x cols = the extent both cover
 * (69 x 1800 in demo mode, 64 x 1792 in batch mode); key_pixels [k_max][2] i64 (row, col), n_key optional device count.
 * ext_pts [k_max * 169][3] f32 out, n_ext [1] i32 out.  ws: caelo_extend_ws_bytes(rows, cols) bytes. */
int64_t caelo_extend_ws_bytes(int rows, int cols);
int caelo_extend_keypts(caelo_ctx *ctx, const float *ring, int ring_w, int ring_c, int32_t *counter, int cnt_w, int rows,
                        int cols, const int64_t *key_pixels, int k_max, const int32_t *n_key, float *ext_pts,
                        int32_t *n_ext, void *ws, void *stream);

/* One iteration of the reference's point-to-point ICP (MyICP.py:26-72; GetPtsInliners :75-85): nearest neighbour in
 * pc0 [n0][3] of every point of pc1 [n1][3] (exact float64 Euclidean distance, first minimum), the pairs closer than
 * `threshold`, SolveRT on them -> rt [12] (R row-major | T, device) and pc1 <- R pc1 + T IN PLACE.  n_inliers [1]
 * (device) = number of pairs; with fewer than min_inliers nothing is fitted or moved (the caller stops: :38-40).
 * Threshold decay and the Euler-angle stop rule stay with the host loop (caelo.api.ICP).  ws: caelo_icp_ws_bytes(n1). */
int64_t caelo_icp_ws_bytes(int64_t n1);
int caelo_icp_step(caelo_ctx *ctx, const float *pc0, int64_t n0, float *pc1, int64_t n1, double threshold, int min_inliers,
                   float *rt, int32_t *n_inliers, void *ws, void *stream);

/* The whole loop of the reference's re-registration on the device:
 *   ICP                    MyICP.py:26-72    use_planar = 0, min_pairs = 100, fail_only_first = 0, threshold0 = 0.5, decay0 = 0.9,
 *                                            small_shift = 0.05, ep = 0.001, max_iter = 50, min_iter = 19
 *   ICP_Pt2PtAndPt2Plane   MyICP.py:127-201  use_planar = 1, min_pairs = 200, fail_only_first = 1 (too few pairs is a failure only in
 *                                            the first iteration), threshold1 / decay1 for the planar gate (caller RefinePoses.py:291-295)
 * pc0 [n0][3], pc1 [n1][3] f32 (pc1 is MOVED in place by every iteration); planar0 [m0][6], planar1 [m1][6] f32 = xyz | normal
 * (planar1's xyz moves, its normals do not: MyICP.py:177).  With use_planar an empty planar set is an error, like sklearn's
 * ValueError at MyICP.py:94 -- GetKeyPtsByAE always returns an empty PlanarPts (SphericalRing.py:219,285).
 * Per iteration: nearest neighbours (exact float64 distance, first minimum) of both sets, the gates, ONE SolveRT over all pairs,
 * R_star / T_star accumulated in float64, the Euler-angle stop rule and the threshold decay -- no host synchronisation; `result`
 * (device) is complete when the stream has passed the call.  ws: caelo_icp_loop_ws_bytes(n1, m1) bytes.
 * From iteration 100 on, ICP_Pt2PtAndPt2Plane fits the planar pairs of iteration 99 alone, as they were then (MyICP.py:151-153:
 * the same (R, T) every time; min_pairs applies to that count and n_inliers_planar keeps it, n_inliers_pts is still counted);
 * ICP goes on as before.  With max_iter = k the result is the loop's state after k iterations.
 * Regime: the reference's use -- up to 50 iterations on a few thousand extended key points.  Every iteration is an exact
 * brute-force nearest-neighbour pass (O(n0 n1) float64 distances) and a one-workgroup update, and ALL max_iter (<= 1000)
 * iterations are enqueued up front (those after convergence return at once): tens of thousands of points or hundreds of
 * iterations work but are not what this entry point is built for.  Nearest-neighbour ties resolve to the lowest index; sklearn's
 * kd-tree (MyICP.py:34-38) makes no promise on exact ties, so clouds with duplicated points may pair differently there. */
typedef struct {
    double threshold0, threshold1, decay0, decay1, small_shift, ep;
    int32_t max_iter, min_iter, min_pairs, fail_only_first, use_planar, reserved;
} caelo_icp_params;
typedef struct {
    double R_star[9], T_star[3];
    double threshold0, threshold1;   /* after the last decay */
    int32_t iterations;              /* iterations that moved pc1 */
    int32_t success;                 /* isSuccess */
    int32_t n_inliers_pts, n_inliers_planar; /* pairs of the last evaluated iteration */
} caelo_icp_result;
int64_t caelo_icp_loop_ws_bytes(int64_t n1, int64_t m1);
int caelo_icp(caelo_ctx *ctx, const float *pc0, int64_t n0, float *pc1, int64_t n1, const float *planar0, int64_t m0, float *planar1,
              int64_t m1, const caelo_icp_params *params, caelo_icp_result *result, void *ws, void *stream);

/* caelo_icp with the nearest-neighbour search over a cell grid: same arguments, parameters and result record, the
 * same pairs in every iteration and so the same bits in `result`, pc1 and planar1 -- built for extended key point sets of 10^5
 * points, where the all-pairs walk of caelo_icp is 10^10 distances an iteration.  Frame 0 (pc0, and planar0 on its own) is binned
 * once per call into cubic cells whose edge is the smallest power of two not below the initial threshold (0.5 -> 0.5, 1.0 -> 1.0,
 * 5.0 -> 8.0); each iteration a frame-1 point visits the 3 x 3 x 3 cells around its own and keeps the minimum by (squared distance,
 * original index), with caelo_icp's distance expression and gate.  The box follows frame 0's extent up to 2^22 cells (2^18 for
 * planar0); points outside it are clamped into its edge cells, which keeps the answer exact.
 * Refused with CAELO_ERR_ARG before any launch, outputs untouched: what caelo_icp refuses; decay0 (and decay1 with use_planar)
 * outside (0, 1] -- a grid built for the initial thresholds cannot answer for larger ones; a threshold that is not positive and
 * finite; a NaN or infinite coordinate in any of the point arrays.  For that check, and to place the box, the arrays are copied
 * to the host first: unlike caelo_icp the call SYNCHRONISES the stream once on entry.
 * ws: 16-byte aligned (the tables are read as 16-byte words; every offset is a multiple of 256), out[7] bytes of
 * caelo_icp_grid_ws_layout(n0, n1, m0, m1, out) (m0 = m1 = 0 without use_planar; CAELO_ERR_ARG for a null out or a size outside [1, 2^30),
 * m0 / m1 from 0); CAELO_ERR_CAPACITY if the host copies for the coordinate check cannot be allocated.  out[0..2] = byte offsets of the
 * cell starts [cells + 1] i32, the cell counters and the (x, y, z, index) table [n0][4] of pc0, out[3..5] the same for planar0,
 * out[6] the scan's chunk totals.  The loop's own record and pair arrays lie in front, as in caelo_icp's workspace. */
int caelo_icp_grid_ws_layout(int64_t n0, int64_t n1, int64_t m0, int64_t m1, int64_t out[8]);
int caelo_icp_grid(caelo_ctx *ctx, const float *pc0, int64_t n0, float *pc1, int64_t n1, const float *planar0, int64_t m0, float *planar1,
                   int64_t m1, const caelo_icp_params *params, caelo_icp_result *result, void *ws, void *stream);

/* ---- evaluation: key point repeatability (EvaluationOnKeypts.py, csrc/evaluate.hip) -----------------------------------------
 * pts [n_frames][ld][3] f64 world-frame key points (device), n_key [n_frames] i32 (device): frame f holds rows 0 .. n_key[f]-1.
 * pairs [n_pairs][2] i32 (device) = (fit frame, query frame).  For every query point: the distance to its nearest fit point, exactly
 * as scikit-learn 0.24.2's kd-tree returns it (minimum of d = 0; d += (x - y)^2 over x, y, z, each operation rounded, then a correctly
 * rounded sqrt) -> dist [n_pairs][ld] f64 (device, nullable; rows past the query frame's n_key are not written).  counts
 * [n_pairs][n_thresholds + 1] i64 (device, overwritten): bin t < T counts #(dist / D_t < 1) - #(dist / D_{t-1} < 1) with an IEEE
 * division, bin T counts #(dist / D_{T-1} >= 1) (EvaluationOnKeypts.py:128-140); a pair (f, f) gives 0 for every point, as the
 * reference's mode 1 does.  thresholds [n_thresholds] f64 (HOST), finite and positive, 1 <= n_thresholds <= 16.
 * The caller validates the data (caelo.Engine.kp_nn_pairs): fit sets of more than 3 points (scikit-learn brute-forces smaller ones),
 * finite coordinates, n_key in [1, ld], pair indices in [0, n_frames).  The kernel clamps n_key to [0, ld] and skips a pair whose
 * index is out of range, so bad data never reads out of bounds. */
#define CAELO_KP_NN_MAX_K 65536
#define CAELO_KP_NN_MAX_THRESHOLDS 16
int caelo_kp_nn_pairs(caelo_ctx *ctx, const double *pts, int64_t n_frames, int ld, const int32_t *n_key, const int32_t *pairs,
                      int64_t n_pairs, const double *thresholds, int n_thresholds, double *dist, int64_t *counts, void *stream);

/* ---- ISS key points: the hand-crafted detector of the key point comparison (PclKeyPts.py:41-46, :92-103; csrc/iss.hip) -----------
 * (additive; the ABI version stays 6.)  The reference calls PCLKeypoint.keypointIss, a PCL binding it does not ship; the model is
 * PCL 1.8's ISSKeypoint3D with border estimation off, the definition is the one below, and bit parity with PCL is
 * not claimed.  pts [n_frames][ld][3] f32 (device), n_pts [n_frames] i32 (device): frame f holds rows 0 .. n_pts[f]-1 (clamped to
 * [0, ld] by the kernels; rows past it are never read into a decision).  All arithmetic is float64, every operation rounded on its
 * own, sums in ascending point index:
 *   neighbours   j is a neighbour of i at radius r <=> d2 < r * r (strict; r * r one rounded product; i is its own neighbour) with
 *                d = double(P[j]) - double(P[i]), d2 = (dx*dx + dy*dy) + dz*dz
 *   scatter      fewer than min_neighbors neighbours at salient_radius: saliency -1, eigenvalues 0; otherwise C_ab = sum_j d_a * d_b
 *                over the neighbours (no division by their number), e1 >= e2 >= e3 its eigenvalues by cyclic Jacobi
 *   candidate    saliency = e3 if e3 >= 0, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (IEEE divisions, a NaN compares false), else -1
 *   key point    saliency > 0, at least min_neighbors neighbours at non_max_radius, none of them with a larger saliency (equal
 *                saliencies both survive)
 * Outputs (device): saliency [n_frames][ld] f64; eig [n_frames][ld][3] f64 = e1, e2, e3 (nullable); n_neigh [n_frames][ld] i32, the
 * neighbours at salient_radius (nullable); key_idx [n_frames][ld] i32, the key points' indices in ascending order, -1 behind them;
 * n_key [n_frames] i32.  Rows n_pts[f] .. ld-1 get saliency -1, eigenvalues 0 and 0 neighbours.  The same input gives the same bits
 * on every run (no atomics); a NaN coordinate only makes comparisons false.  Three kernels, each one launch for all frames (the
 * all-pairs passes in slices of 65 535 frames); ws: caelo_iss_ws_bytes(n_frames, ld) bytes, no initialisation, one per call in flight.
 * prm is HOST memory.  Refused before any launch (CAELO_ERR_ARG): null arguments, ld outside [1, CAELO_ISS_MAX_POINTS], radii or gammas
 * that are not finite and positive, min_neighbors < 1, a short workspace.  n_frames == 0 is a no-op.  The call does not synchronise.
 * The work is n_pts^2 pair distances per frame and pass: 16 384 points (the reference's input_pc_num) are the intended size. */
#define CAELO_ISS_MAX_POINTS 32768
typedef struct { double salient_radius, non_max_radius, gamma_21, gamma_32; int32_t min_neighbors, reserved; } caelo_iss_params;
int64_t caelo_iss_ws_bytes(int64_t n_frames, int ld);
int caelo_iss_keypoints(caelo_ctx *ctx, const float *pts /*[n_frames][ld][3] device*/, int64_t n_frames, int ld,
                        const int32_t *n_pts /*[n_frames] device*/, const caelo_iss_params *prm /*host*/,
                        double *saliency /*[n_frames][ld]*/, double *eig /*[n_frames][ld][3] e1,e2,e3; nullable*/,
                        int32_t *n_neigh /*[n_frames][ld] at salient_radius; nullable*/,
                        int32_t *key_idx /*[n_frames][ld]*/, int32_t *n_key /*[n_frames]*/,
                        void *ws, int64_t ws_bytes, void *stream);

/* ---- Harris3D key points: the second hand-crafted detector of the key point comparison (PclKeyPts.py:50-51, :63; csrc/harris.hip) --
 * (additive; the ABI version stays 6.)  The reference calls PCLKeypoint.keypointHarris; the model is PCL 1.8's HarrisKeypoint3D, method
 * HARRIS, non-maximum suppression on, refinement off, normals from NormalEstimation at the same radius.  The definition is the one
 * below, and bit parity with PCL is not claimed.  pts, n_pts: as for caelo_iss_keypoints.  All arithmetic is float64,
 * every operation rounded on its own (IEEE division and square root), sums in ascending point index:
 *   neighbours   as in ISS: j is a neighbour of i <=> d2 < radius * radius (strict; one rounded product; i is its own neighbour)
 *   normal       k neighbours; k < 3: invalid.  Otherwise S_a = sum d_a and S_ab = sum d_a * d_b over the neighbours (nine sums in one
 *                pass), C_ab = S_ab - (S_a * S_b) / double(k); the normal is the unit eigenvector of C's smallest eigenvalue: the cyclic
 *                Jacobi of the ISS eigenvalues (same rotation order, formulas, skip rule, 12-sweep bound) with the rotations
 *                accumulated into V from the identity, the column of the smallest diagonal entry (lowest index on a tie) divided by
 *                sqrt((x*x + y*y) + z*z) -- a pure function of the six entries; a row and column that are exactly zero keep their
 *                unit vector exactly.  If (n_x*p_x + n_y*p_y) + n_z*p_z > 0 the normal is negated: it faces the sensor at the origin.
 *                Nothing below depends on the sign.
 *   response     invalid normal: -1.  Otherwise c = the neighbours with a valid normal (>= 1: the point itself),
 *                N_ab = (sum n_a * n_b) / double(c) over them for (xx, xy, xz, yy, yz, zz), tr = (N_xx + N_yy) + N_zz,
 *                det = (((N_xx*N_yy)*N_zz + (2*N_xy)*N_xz*N_yz) - (N_xz*N_xz)*N_yy - (N_xy*N_xy)*N_zz) - (N_yz*N_yz)*N_xx, left to
 *                right; response = (0.04 + det) - (0.04*tr)*tr if tr != 0, else 0 (PCL's expression; in [0, 1/27] to rounding)
 *   key point    valid normal, response >= threshold, and no neighbour j with a valid normal has response[i] < response[j] (equal
 *                responses both survive)
 * Outputs (device): response [n_frames][ld] f64; normals [n_frames][ld][3] f64 (nullable); n_neigh [n_frames][ld] i32 (nullable);
 * key_idx [n_frames][ld] i32, the key points' indices in ascending order, -1 behind them; n_key [n_frames] i32.  Rows n_pts[f] .. ld-1
 * get response -1, normal 0 and 0 neighbours.  The same input gives the same bits on every run and in every batch composition (no
 * atomics, no cross-thread sums); a NaN coordinate only makes comparisons false.  Four kernels, each one launch for all frames (the
 * three all-pairs passes in slices of 65 535 frames); ws: caelo_harris_ws_bytes(n_frames, ld) bytes, no initialisation, one per call
 * in flight.  prm is HOST memory.  Refused before any launch (CAELO_ERR_ARG): null arguments, ld outside [1, CAELO_ISS_MAX_POINTS],
 * n_frames < 0, a radius that is not finite and positive, a threshold that is not finite or is negative, a short workspace.
 * n_frames == 0 is a no-op.  The call does not synchronise.  The work is n_pts^2 pair distances per frame and pass. */
typedef struct { double radius, threshold; } caelo_harris_params;
int64_t caelo_harris_ws_bytes(int64_t n_frames, int ld);
int caelo_harris_keypoints(caelo_ctx *ctx, const float *pts /*[n_frames][ld][3] device*/, int64_t n_frames, int ld,
                           const int32_t *n_pts /*[n_frames] device*/, const caelo_harris_params *prm /*host*/,
                           double *response /*[n_frames][ld]*/, double *normals /*[n_frames][ld][3]; nullable*/,
                           int32_t *n_neigh /*[n_frames][ld]; nullable*/,
                           int32_t *key_idx /*[n_frames][ld]*/, int32_t *n_key /*[n_frames]*/,
                           void *ws, int64_t ws_bytes, void *stream);

/* ---- SIFT3D key points: the third hand-crafted detector of the key point comparison (PclKeyPts.py:55-58, :63; csrc/sift.hip) -------
 * (additive; the ABI version stays 6.)  The reference calls PCLKeypoint.keypointSift; the model is PCL 1.8's SIFTKeypoint on PointXYZ
 * with the point's z coordinate as the filtered field.  The definition is the one below, and bit parity with PCL is not
 * claimed.  caelo_sift_octave is ONE octave: a cloud per frame and a list of scales; the pyramid over the octaves (voxel-grid
 * centroids at leaf min_scale * 2^o, the scales of an octave, the stop under 25 points) is the caller's (caelo.Engine.sift_keypoints).
 * pts, n_pts: as for caelo_iss_keypoints.  All arithmetic is float64, every operation rounded on its own (IEEE division), sums in
 * ascending point index; the one exception is exp, the device's float64 exp, which is not correctly rounded:
 *   scale space  value_j = double(P[j].z); d = double(P[j]) - double(P[i]), d2 = (dx*dx + dy*dy) + dz*dz.  For every scale s:
 *                j counts <=> d2 <= 9.0 * (sigma[s]*sigma[s]) (not strict; two rounded products; i counts itself with w = 1),
 *                w = exp((-0.5 * d2) / (sigma[s]*sigma[s])), num_s = sum value_j * w, den_s = sum w, resp_s = num_s / den_s,
 *                dog[i][s] = resp_{s+1} - resp_s for s = 0 .. D-1, D = n_scales - 1
 *   neighbours   the CAELO_SIFT_K points with the smallest (d2, j) in lexicographic order, the point itself included (ties in
 *                distance go to the lower index); a frame of fewer than CAELO_SIFT_K points has no key points, its dog is still written
 *   key point    for s = 1 .. D-2, v = dog[i][s], mn[t] / mx[t] the minimum / maximum of dog[j][t] over the neighbours: (i, s) is a key
 *                <=> |v| >= min_contrast and (v == mn[s] && v < mn[s-1] && v < mn[s+1]  ||  v == mx[s] && v > mx[s-1] && v > mx[s+1])
 *                (equal values at the same level both survive)
 * Outputs (device): dog [n_frames][ld][D] f64; knn [n_frames][ld][CAELO_SIFT_K] i32 in (d2, j) order, -1 behind a frame's points when
 * it has fewer (nullable); key_mask [n_frames][ld] u32, bit s set for every key (i, s); key_idx [n_frames][ld] i32, the points with a
 * non-zero mask in ascending order, -1 behind them; n_key [n_frames] i32.  Rows n_pts[f] .. ld-1 get dog 0, knn -1 and mask 0.  The
 * same input gives the same bits on every run and in every batch composition (no atomics, no cross-thread sums); a NaN coordinate only
 * makes comparisons false.  Four kernels, each one launch for all frames (the three per-point passes in slices of 65 535 frames); ws:
 * caelo_sift_ws_bytes(n_frames, ld) bytes, no initialisation, one per call in flight.  prm is HOST memory.  Refused before any launch
 * (CAELO_ERR_ARG): null arguments, ld outside [1, CAELO_ISS_MAX_POINTS], n_frames < 0, n_scales outside [3, CAELO_SIFT_MAX_SCALES],
 * scales that are not finite, positive and increasing, a min_contrast that is not finite or is negative, a short workspace.
 * n_frames == 0 is a no-op.  The call does not synchronise.  The work is n_pts^2 pair distances per frame in each all-pairs pass.
 *
 * caelo_voxel_centroids: the centroids of a voxel grid's cells, which the pyramid is built from.  pts [n_pts][3] f32; order [n_pts]
 * i32, the rows stably sorted by cell; starts [n_cells + 1] i32, where each cell's run of `order` begins (all device; the caller sorts:
 * caelo.Engine.voxel_centroids, cells = floor(double(p) / leaf) ordered by (cz, cy, cx)).  Each coordinate of centroids [n_cells][3]
 * f32 is the float64 sum over the cell's run in the order given (ascending input row under a stable sort) divided by double(count),
 * rounded to float32.  An index outside [0, n_pts) is skipped and a run is clamped to the list, so bad lists never read out of bounds. */
#define CAELO_SIFT_K 25
#define CAELO_SIFT_MAX_SCALES 19
typedef struct { int32_t n_scales, reserved; double min_contrast; double sigma[CAELO_SIFT_MAX_SCALES]; } caelo_sift_params;
int64_t caelo_sift_ws_bytes(int64_t n_frames, int ld);
int caelo_sift_octave(caelo_ctx *ctx, const float *pts /*[n_frames][ld][3] device*/, int64_t n_frames, int ld,
                      const int32_t *n_pts /*[n_frames] device*/, const caelo_sift_params *prm /*host*/,
                      double *dog /*[n_frames][ld][n_scales-1]*/, int32_t *knn /*[n_frames][ld][CAELO_SIFT_K]; nullable*/,
                      uint32_t *key_mask /*[n_frames][ld]*/, int32_t *key_idx /*[n_frames][ld]*/, int32_t *n_key /*[n_frames]*/,
                      void *ws, int64_t ws_bytes, void *stream);
int caelo_voxel_centroids(caelo_ctx *ctx, const float *pts /*[n_pts][3]*/, int64_t n_pts, const int32_t *order /*[n_pts]*/,
                          const int32_t *starts /*[n_cells + 1]*/, int64_t n_cells, float *centroids /*[n_cells][3]*/, void *stream);

/* ---- frame pipeline: batches of frames behind single launches, three stages on three HIP streams ------------------
 * Replaces the reference's per-frame driver loops (BatchPreprocess.py:88-140 extract loop, Match.py:296-353 /
 * PoseEstimation.py pair loop) for throughput.  `batch` consecutive frames share ONE launch of every kernel of the
 * front half of caelo_extract (ring image, response, keypoints, voxel map, patch gather), one encoder launch set and
 * one caelo_match / caelo_ransac launch per threshold level; front(b+1), encoder(b) and pairs(b-1) overlap on three
 * streams.  Per-frame results are identical to the single-call entry points (same kernels, same per-frame arithmetic).
 *   create(ctx, batch in [1,8], n_buffers in [2,4], max_points)   n_buffers = batches of patches in flight between
 *                                                                   the front and the encoder
 *   begin(stream)   the stages wait for work already queued on `stream` (the producers of the jobs' inputs)
 *   submit(job)     copy the job; every `batch` jobs (or when the mode changes) the batch is launched:
 *                     caelo_extract(pc -> rows [1024][64] = descriptor 0:60 | xyz 60:63 | valid 63, ...)
 *                     pair == CAELO_PAIR_CHAIN:    caelo_match + caelo_ransac against the previously submitted frame
 *                     pair == CAELO_PAIR_EXPLICIT: ... against prev_rows / prev_n_key (e.g. rows gathered from a peer)
 *   flush(stream)   launch a partial batch, make `stream` wait for all three stages
 * Buffers named by a job must stay alive until `stream` has passed the flush.  Calls come from ONE host thread.
 * A failed launch is returned by the submit / flush that issued it (caelo_last_error() holds the text). */
typedef struct caelo_pipeline caelo_pipeline;
#define CAELO_PAIR_NONE 0
#define CAELO_PAIR_CHAIN 1
#define CAELO_PAIR_EXPLICIT 2
typedef struct caelo_frame_job {
    const float *pc;            /* [n][4] f32 */
    int64_t n;
    int32_t dist_channels;      /* 5 | 3, see caelo_extract */
    int32_t mode;               /* CAELO_EXTRACT_* bits (CAELO_EXTRACT_EXACT_PATCHES: the reference's patches, see caelo_extract; the
                                   status word then also reports CAELO_ST_TIES_LEFT.  The first job in this mode allocates, before its batch
                                   is launched, the kd storage and ordering scratch of every frame slot's map -- per slot what caelo_extract
                                   lists, and on slot 0 the batch's sort buffers, batch x 3 x max_points x 24 B) */
    float *rows;                /* [1024][64] f32 out */
    int64_t *key_pixels;        /* [1024][2] out */
    int32_t *n_key;             /* [1] out */
    uint8_t *flags;             /* [1024][3] out */
    int32_t *status;            /* int32[4], 16-byte aligned, out */
    int32_t pair;               /* CAELO_PAIR_* */
    int32_t reserved;
    const float *prev_rows;     /* CAELO_PAIR_EXPLICIT: [1024][64] rows of frame 0 of the pair */
    const int32_t *prev_n_key;  /* CAELO_PAIR_EXPLICIT: its keypoint count (NULL = 1024) */
    const double *rand;         /* [1500][4] f64 uniform draws (caelo_ransac) */
    caelo_pose_result *result;  /* out */
    uint8_t *inlier_mask;       /* [1024] out */
    int64_t *pair_idx;          /* [1024] out */
    caelo_ransac_cert *cert;    /* out, nullable: the pair's certificate for caelo_host_certify */
    /* The host half inside the pipeline (needs caelo_host_bind_blas): when result_host is given, the kernels write the pair's
     * certificate straight into pinned host memory of the pipeline (`cert` is not used; CAELO_CERT_ZEROCOPY=0: into `cert`, copied by
     * a copy command), the issuing thread finds the pair stage finished two batches later (no device-side wait), certifier threads
     * run the host half while later batches are on the GPU and write the EXACT result -- the reference's
     * inlier set, R_star / T_star, refit, bit for bit -- to these HOST buffers; caelo_pipeline_flush returns when all are written.
     * The kernels then stop at the certificate: `result` and `inlier_mask` (device) are NOT written for such a pair -- the winner,
     * mask and refit k_ransac_finish would compute are exactly what the host half replaces. */
    caelo_pose_result *result_host; /* out, nullable */
    uint8_t *mask_host;             /* [1024] out (required with result_host) */
    const double *rand_host;        /* nullable: host copy of `rand` (only read when the pair escalates beyond 0.4 m; fetched from `rand` otherwise) */
    int32_t *info_host;             /* nullable: [2] = hypotheses evaluated on the host, status (0 exact, 2 no bounds, 3 no record) */
} caelo_frame_job;
int caelo_pipeline_create(caelo_ctx *ctx, int batch, int n_buffers, int64_t max_points, caelo_pipeline **out);
/* host half inside the pipeline: out_host[4] = pairs certified, hypotheses evaluated for them, nanoseconds of the certifier thread, nanoseconds the issuing thread spent handing certificates over -- since the last call */
int caelo_pipeline_cert_stats(caelo_pipeline *pipe, int64_t *out_host);
void caelo_pipeline_destroy(caelo_pipeline *pipe);
int caelo_pipeline_batch(const caelo_pipeline *pipe);
int caelo_pipeline_begin(caelo_pipeline *pipe, void *stream);
int caelo_pipeline_submit(caelo_pipeline *pipe, const caelo_frame_job *job);
/* n jobs in one call (the same as n caelo_pipeline_submit calls in order; stops at the first error): a host language with a
 * costly foreign-call path (ctypes: ~10 us per call) hands a whole run over at once -- the odometry loop of PoseEstimation.py:241-267. */
int caelo_pipeline_submit_many(caelo_pipeline *pipe, const caelo_frame_job *jobs, int64_t n);
int caelo_pipeline_flush(caelo_pipeline *pipe, void *stream);
/* Results that leave while the pipeline runs -- the sharded sequence's descriptor all-gather (PoseEstimation.py:241-251 needs the
 * previous frame's features wherever that frame was extracted): `stream` waits until the rows (descriptors | key points | valid)
 * of every frame of the batches ISSUED so far are written, and of nothing later -- a collective enqueued on `stream` then moves
 * finished rows while the next batches are still being extracted.  Between caelo_pipeline_begin and caelo_pipeline_flush. */
int caelo_pipeline_wait_encoded(caelo_pipeline *p, void *stream);
/* The same hand-over paced by the host: blocks the calling thread until the rows of every batch issued so far except the last
 * `lag` (0 <= lag < buffers) are written; work enqueued afterwards on any stream of this device may read them without a
 * device-side wait.  With lag >= 1 the pipeline keeps `lag` batches queued behind the one being waited for. */
int caelo_pipeline_sync_encoded(caelo_pipeline *p, int lag);
/* Pacing of the issuing thread: after issuing a batch, caelo_pipeline_submit waits until the batch `lag` before it is through the
 * encoder (default 1, or CAELO_PIPE_PACE; -1: never waits, the thread runs as far ahead as the queues take).  Waits that sit
 * unsatisfied in the hardware queues cost throughput, and a thread running far ahead leaves many: 16.5 k -> 17.3 k frames/s on
 * a 20-batch run.  A caller that paces itself (caelo_pipeline_sync_encoded between its own work) turns this off. */
int caelo_pipeline_set_pace(caelo_pipeline *p, int lag);
int caelo_pipeline_get_pace(const caelo_pipeline *p);   /* the pacing in effect (the library's default until set) */
/* The HIP streams of the stages: out_host[4] = front, encoder, pair, voxel maps.  Stages that share a stream report the same handle;
 * out_host[3] is null when the voxel maps are built on the front stream.  (Tests hold one stage back to check the hand-offs.) */
int caelo_pipeline_streams(const caelo_pipeline *p, void **out_host);
/* Read-only, for tests: copies `bytes` bytes at `offset` of the extract workspace of frame slot i of a batch to the device buffer `dst`,
 * on `stream`.  The workspace is laid out as caelo_extract's (caelo_extract_ws_kp_eligible_offset(), caelo_extract_ws_ring_offset()).
 * The copy is ordered by `stream` alone: the caller makes `stream` wait for the pipeline's front stage first -- the stream a run
 * was flushed on (caelo_pipeline_flush) has waited for every stage -- and lets no later batch be issued before the copy is done. */
int caelo_pipeline_extract_ws_read(const caelo_pipeline *p, int i, int64_t offset, int64_t bytes, void *dst, void *stream);
/* n host -> device copies on `stream` behind one call (the scans of a batch that live in pinned host memory, the producer side of
 * PoseEstimation.py:214-245): dst[i] <- src[i], bytes[i] each, asynchronous like hipMemcpyAsync; a null dst[i] or src[i] is an error,
 * a zero bytes[i] is skipped.  The pipeline does not take part -- the caller orders the copies against it (an event of its own,
 * caelo_pipeline_sync_encoded); caelo_pipeline_run_uploading issues each batch's copies through it. */
int caelo_upload_many(void *const *dst, const void *const *src, const size_t *bytes, int n, void *stream);
/* A whole run of the upload mode behind ONE call: jobs [k] (in nb batches of the pipeline's batch size, the remainder last) whose
 * scans arrive on `copy_stream`, `ahead` batches ahead of the batch being issued; the calling thread waits for a batch's arrival,
 * submits it, queues the next batch's copies and paces itself one batch behind the encoder -- natively: the interpreter's ~60 us
 * between that wait and the next batch's front launches were 20 % of the rate.  Includes caelo_pipeline_begin and the flush (the
 * pipeline's pacing is off during the call and restored after it).  Without a loader: a copy table -- batch b is uploaded by the
 * entries [copy_first[b], copy_first[b + 1]) of dst / src / bytes (caelo_upload_many), copy_first [nb + 1] non-decreasing from 0:
 * one entry per batch when a batch's scans lie in one block at a fixed pitch (one copy command per batch: several commands per batch
 * cost a pipeline running beside them 20 %), one per frame otherwise.  With a loader (caelo_seqloader, below; copy_first unused):
 * batch b0 + b comes from its ring slot (ring_host, slot_bytes) into dst[(b0 + b) % n_slots] (n_slots >= ahead + 2 device slots of
 * slot_bytes), and the point counts of its jobs (job.n) are filled in from the loader, which gets its slot back as soon as the copy is
 * through.  A device slot is overwritten only after the previous batch in it is through its pair stage, which reads the draws there
 * (the calling thread waits for an event on the pair stream; without a loader only the front stage reads a slot, and the wait for the
 * encoder covers it).  Jobs that take their host draws from the loader's keep ring (rand_host, certified) need keep_batches >=
 * ring_batches + 7: the certifier may still read a batch's draws while the loader refills up to ring_batches + 6 batches later.
 * times_ns_host (nullable) [4]: waiting for the loader / for arrivals, submitting, copy issue + pacing. */
struct caelo_seqloader;
int caelo_pipeline_run_uploading(caelo_pipeline *pipe, caelo_frame_job *jobs, int64_t k, int64_t nb, struct caelo_seqloader *loader, int64_t b0,
                                 void *const *dst, const void *const *src, const size_t *bytes, const int64_t *copy_first, int n_slots,
                                 const void *ring_host, int64_t slot_bytes, int ahead, void *copy_stream, void *stream, int64_t *times_ns_host);

/* ---- a sequence from files (PoseEstimation.py:173-245: the generator process that prepares frame i + 1 while frame i is matched) ----
 * caelo_host_random_sample: numpy.random.RandomState(seed).random_sample(n) bit for bit (MT19937, init_genrand seeding, 53-bit doubles):
 * the stream RANSAC4RT draws its samples from (Match.py:182-184), CAELO_SEQ_DRAWS doubles per pair (3 levels x 500 trials x 4).
 * caelo_seqloader: `threads` native threads read the n KITTI .bin files of `paths` ([points][4] f32) batch after batch into the caller's
 * (pinned) ring of `ring_batches` slots.  A slot (caelo_seqloader_slot_bytes) = [batch][cap_points][4] f32 scans, then
 * [batch][CAELO_SEQ_DRAWS] f64 draws -- file i's are those of pair (frame - 1, frame) = RandomState(seed_base + first_frame + i - 1) -- so
 * that one copy command moves a batch to a device slot of the same layout; draws_keep_host (nullable) [keep_batches][batch][CAELO_SEQ_DRAWS]
 * keeps batch b's draws at b % keep_batches for the host half (caelo_frame_job::rand_host).  _wait blocks until batch b (files b * batch ..)
 * sits in slot b % ring_batches and reports the point counts; _release hands the slot back (in order).  A file that is missing, not a
 * multiple of 16 bytes or larger than a slot fails the wait with an error naming it.  RandomState takes seeds in [0, 2^32): a
 * seed_base that gives a frame WITH a pair (global frame index >= 1) a seed outside that range is refused.  Host code only. */
#define CAELO_SEQ_DRAWS (CAELO_RANSAC_LEVELS * CAELO_RANSAC_MAX_TRIALS * 4)
typedef struct caelo_seqloader caelo_seqloader;
int caelo_host_random_sample(uint32_t seed, int64_t n, double *out_host);
int64_t caelo_seqloader_slot_bytes(int batch, int64_t cap_points);
int caelo_seqloader_create(const char *const *paths, int64_t n, int64_t first_frame, int batch, int ring_batches, int64_t cap_points,
                           void *ring_host, double *draws_keep_host, int keep_batches, int64_t seed_base, int threads, caelo_seqloader **out);
int caelo_seqloader_wait(caelo_seqloader *loader, int64_t b, int32_t *slot_host, int64_t *n_points_host);
int caelo_seqloader_release(caelo_seqloader *loader, int64_t b);
int caelo_seqloader_stats(caelo_seqloader *loader, int64_t *out_host);   /* [3]: ns reading, drawing, waiting for a slot (summed over threads) */
void caelo_seqloader_destroy(caelo_seqloader *loader);
/* host-side counters since the last call (then reset): out_host[6] = jobs, ns the calling thread spent issuing their
 * launches, batches launched, batch size, hand-off buffers, HIP streams used */
/* Optional hint before caelo_pipeline_begin: the run will submit n_frames jobs.  If that is not a multiple of the batch size, the
 * frames are spread evenly over ceil(n_frames / batch) batches (20 on batch 8: 6 + 7 + 7) instead of full batches and a
 * remainder -- nothing overlaps the first batch's front stage nor the last batch's encoder + pair stages, so neither should be
 * the odd one out.  The hint holds for one run (cleared by caelo_pipeline_flush); results do not depend on it. */
int caelo_pipeline_expect(caelo_pipeline *pipe, int64_t n_frames);
int caelo_pipeline_stats(caelo_pipeline *pipe, int64_t *out_host);

/* ---- pair tables: the pipeline's pair stage over ANY frame pairs of resident rows (additive; the ABI version stays 6) -------------
 * The pipeline registers frame i against frame i + 1.  caelo_register_pairs registers a table pairs [n_pairs][2] i32 of
 * (frame 0, frame 1) indices into rows [n_frames][1024][64] f32 (a pipeline's rows: descriptor 0:60 | xyz 60:63 | valid 63,
 * 16-byte aligned) with n_key [n_frames] i32 -- all DEVICE memory, as written by work queued on `stream` before the call.  The
 * kernels are the pair stage's own (NN match with the float64 certification of the argmin, the 500 hypotheses of the 0.4 m level,
 * the bounds of the 0.8 / 1.6 m levels, the refit) taking their pairs from the table: a pair gives the bits it gives in a pipeline
 * batch and through caelo_match + caelo_ransac.  Pair q draws from rand + q * 6000 ([n_pairs][3 * 500][4] f64, device) and writes
 *   pair_idx_out [n_pairs][1024] i64, and
 *   results_out [n_pairs] + masks_out [n_pairs][1024] u8: the kernels' float64 fits and inlier masks, and / or
 *   certs_out [n_pairs] (16-byte aligned): the certificates, which caelo_host_certify takes unchanged once copied to the host.
 * results_out and masks_out go together; both null with certs_out given: certificates only, the host half produces the results
 * (the finishing kernel is not launched, as in a pipeline job with result_host).
 * A launch of every kernel covers up to 8 pairs; larger tables are walked in such slices, ordered by (frame 0, frame 1) so that
 * pairs sharing a frame sit in one launch (outputs stay in the table's order).  ws: caelo_register_pairs_ws_bytes(n_pairs) bytes (eight slots of match + RANSAC workspace),
 * 16-byte aligned, no initialisation, one per call in flight; no other device memory is allocated.
 * Refused before any launch (CAELO_ERR_ARG, caelo_last_error): a null table, a frame index outside [0, n_frames), a frame of the
 * table whose n_key lies outside [1, 1024].  The call waits for `stream` once (it reads the table and the counts back to check
 * them: one hipStreamSynchronize, nothing is uploaded); the results are complete when `stream` has passed the call.  A pair (f, f) is
 * legal: every point matches the FIRST point with its descriptor (itself unless descriptors repeat, Match.py:258) and the pose is the
 * identity to float32 rounding. */
int64_t caelo_register_pairs_ws_bytes(int64_t n_pairs);
int caelo_register_pairs(caelo_ctx *ctx, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs,
                         const double *rand, int64_t *pair_idx_out, caelo_pose_result *results_out, uint8_t *masks_out,
                         caelo_ransac_cert *certs_out, void *ws, void *stream);

/* caelo_register_pairs on descriptors of the caller's: desc [n_frames][1024][ld_desc] f32 (device, ld_desc >= dim floats per key
 * point, 1 <= dim <= 256) replaces columns 0:60 of the rows in the NN match; the rows still supply xyz (60:63) and n_key the
 * counts, and their columns 0:60 are not read.  Everything else is caelo_register_pairs: slices of 8 pairs ordered by
 * (frame 0, frame 1), the checks before any launch, results and / or certificates.  The match of a slice is caelo_match's for that
 * width (dim <= 62 the f16 screen, 63 / 64 the float64 kernel, wider the screen over several blocks) over the slice's pairs in ONE
 * launch set; desc = rows with ld_desc 64 and dim 60 gives caelo_register_pairs' bits.
 * ws: caelo_register_pairs_ws_bytes_dim(n_pairs, dim) bytes (caelo_register_pairs_ws_bytes' figure for dim <= 64). */
int64_t caelo_register_pairs_ws_bytes_dim(int64_t n_pairs, int dim);
int caelo_register_pairs_desc(caelo_ctx *ctx, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs,
                              const double *rand, int64_t *pair_idx_out, caelo_pose_result *results_out, uint8_t *masks_out,
                              caelo_ransac_cert *certs_out, void *ws, void *stream, const float *desc, int64_t ld_desc, int dim);

/* ---- the comparison protocol's registrar (additive; the ABI version stays 6) ---------------------------------------------------------
 * The reference's published table was written by Scripts/GenerateTrajactory.m, which registers with External/ransacfitRt.m and not with
 * Match.py: 3-point samples, a quaternion least-squares fit (estimateRigidTransform.m + quat2rot.m), ONE inlier threshold (1.0 m
 * there), an adaptive trial count (ransac.m: p = 0.99, at least 100 trials, the identity after 10 000), `>=` when a new best is
 * recorded (among equal counts the LATER trial wins) and a least-squares refit on the best trial's inliers.  float64 throughout.
 * Pairs: p0[i] ~ R p1[i] + T, i < n <= 1024.  Trial t samples three DISTINCT pairs from draws[t][0:3] (uniform doubles in [0, 1);
 * draws [CAELO_ADAPTIVE_DRAWS][3] f64; this sample rule is the project's own, MATLAB's randsample stream cannot be reproduced):
 *   i0 = min(floor(u0 n), n - 1);  j1 = min(floor(u1 (n - 1)), n - 2), i1 = j1 + (j1 >= i0);
 *   j2 = min(floor(u2 (n - 2)), n - 3), i2 = j2 + (j2 >= min(i0, i1)), one more if that is >= max(i0, i1).
 * status 0: R, T the refit, R_ransac, T_ransac the best trial, best_trial its index, trials the script's trialcount; with fewer than 3
 *   inliers R, T are the identity and n_inliers 0 (ransacfitRt.m:43-50).  n == 3: the direct fit, all three inliers, 0 trials,
 *   best_trial -1.
 * status 1: the walk ran into the limit: the identity, no inliers, trials = 10 000, best_trial -1.
 * status 2: n < 3: the identity, no inliers, 0 trials.
 * caelo_ransac_adaptive: p0, p1 [n][3] f64, draws, result and mask [n] u8 are DEVICE memory; one workgroup; ws is not used (may be
 *   null).  Nothing is read back, nothing waits.
 * caelo_host_ransac_adaptive: the same functions compiled for the host on HOST arrays; no device is touched.  The trial fits are the
 *   kernel's operation for operation; the refit adds its inliers in index order where the kernel adds them as a tree.
 * caelo_register_pairs_adaptive: caelo_register_pairs_desc's arguments with draws and threshold in place of rand, and no certificates
 *   (desc null: the rows' columns 0:60).  The match direction is the script's, the OTHER way round from caelo_register_pairs: for each
 *   key point i of frame a = pairs[q][0] the nearest descriptor of frame b = pairs[q][1] (the float64 argmin, first index on ties:
 *   caelo_match with the two frames exchanged), so pair_idx_out [n_pairs][1024] indexes frame B, there are n_key[a] pairs, and
 *   masks_out [n_pairs][1024] is over frame A's points (caelo_register_pairs: pair_idx indexes frame 0, the mask is over frame 1).
 *   The pose still maps frame b into frame a.  Every pair consumes the same draws (ransac.m resets its stream per call).  The same
 *   refusals before any launch and the same single wait for `stream` as caelo_register_pairs; the match runs in slices of 8 pairs, then
 *   ONE launch registers all pairs, a workgroup each.  ws: caelo_register_pairs_adaptive_ws_bytes(n_pairs, dim) bytes, 16-byte aligned. */
#define CAELO_ADAPTIVE_MAX_TRIALS 10000
#define CAELO_ADAPTIVE_DRAWS (CAELO_ADAPTIVE_MAX_TRIALS + 1)
typedef struct {
    double R[9], T[3];                 /* refit */
    double R_ransac[9], T_ransac[3];   /* best trial */
    int32_t n_pairs, n_inliers, trials, best_trial;
    int32_t status;                    /* 0 ok, 1 trial limit, 2 fewer than 3 pairs */
    int32_t reserved;
} caelo_adaptive_result;
int caelo_ransac_adaptive(caelo_ctx *ctx, const double *p0, const double *p1, int64_t n, const double *draws, double threshold,
                          caelo_adaptive_result *result, uint8_t *mask, void *ws, void *stream);
int caelo_host_ransac_adaptive(const double *p0_host, const double *p1_host, int64_t n, const double *draws_host, double threshold,
                               caelo_adaptive_result *result_host, uint8_t *mask_host);
int64_t caelo_register_pairs_adaptive_ws_bytes(int64_t n_pairs, int dim);
int caelo_register_pairs_adaptive(caelo_ctx *ctx, const float *rows, int64_t n_frames, const int32_t *n_key, const int32_t *pairs, int64_t n_pairs,
                                  const double *draws, double threshold, int64_t *pair_idx_out, caelo_adaptive_result *results_out,
                                  uint8_t *masks_out, void *ws, void *stream, const float *desc, int64_t ld_desc, int dim);

/* ---- planar points with normals (additive; the ABI version stays 6; csrc/planar.hip) -----------------------------------
 * What ICP_Pt2PtAndPt2Plane registers with (RefinePoses.py:291-294; caelo_icp / caelo_icp_grid with use_planar): the producer written
 * down in GetKeyPtsByAE's commented per-pixel loop (SphericalRing.py:236-282).  Inputs as for caelo_keypoints: ring [>=64][ring_w][ring_c]
 * f32 (ring_c 3 or 5), counter [>=64][cnt_w] i32 (occupied = counter > 0), resp [64][1792][8] f32.  For every pixel of rows 8..55 and
 * columns 8..1783 (:64-68) in row-major order:
 *   1. the pixel is occupied (:243);  2. its 5 x 5 window holds at least 5 occupied pixels beside it (:246-250);
 *   3. minDiff = the minimum over those of the float32 L2 norm of the response difference (caelo_keypoints' arithmetic; a NaN among
 *      them stays a NaN and fails every comparison);
 *   4. if (double)minDiff > 0.2 and the float32 norm of the centre's x, y, z is < 10 the pixel is skipped (:259-262);
 *   5. (double)minDiff < 0.4 (:268, PlanarThreshold :129);
 *   6. the float64 covariance (mean = sum / N, centred second moments / (N - 1), summed in window order) of the x, y, z of the
 *      occupied window pixels without the centre (:269-271), the eigenvector of its smallest eigenvalue by a cyclic Jacobi, the
 *      first one among equal eigenvalues (:272-274);
 *   7. |n_z| > 0.9 (:275) -> the row [x, y, z, n_x, n_y, n_z] (:276): the point's float32 bits, the normal rounded to float32, its
 *      sign chosen so that n_z > 0 (LAPACK's is arbitrary; the ICP multiplies by the normal twice and does not depend on it).
 * A non-finite coordinate in a window makes the covariance NaN and the pixel fails 7.
 * planar [CAELO_PLANAR_MAX][6] f32, pixels [CAELO_PLANAR_MAX][2] i32 (row, col; may be NULL), n_planar [1] i32: rows 0 .. n_planar - 1 are
 * written, in row-major pixel order, the rows behind them are left alone.  No atomic decides a position: the same input gives the
 * same bytes on every run.
 * caelo_planar_points: device memory; two launches on `stream`, nothing is read back, nothing waits.  ws: caelo_planar_ws_bytes()
 *   bytes, 16-byte aligned, no initialisation needed.  Refused before any launch (CAELO_ERR_ARG): a null argument (but pixels), ring_w or
 *   cnt_w below 1792, ring_c other than 3 or 5, a ws that is not 16-byte aligned.
 * caelo_host_planar_points: the same per-pixel function compiled for the host, looped over HOST arrays; no context, no device. */
#define CAELO_PLANAR_MAX (48 * 1776)
int64_t caelo_planar_ws_bytes(void);
int caelo_planar_points(caelo_ctx *ctx, const float *ring, int ring_w, int ring_c, const int32_t *counter, int cnt_w, const float *resp,
                        void *ws, float *planar, int32_t *pixels, int32_t *n_planar, void *stream);
int caelo_host_planar_points(const float *ring_host, int ring_w, int ring_c, const int32_t *counter_host, int cnt_w, const float *resp_host,
                             float *planar_host, int32_t *pixels_host, int32_t *n_planar_host);

/* ---- loop closure: Scan Context descriptors and the all-pairs shifted search (additive; the ABI version stays 6; csrc/loopclose.hip,
 * DESIGN.md 9n).  Kim & Kim, "Scan Context", IROS 2018; the definitions below are this library's own (tests/loops_ref.py restates them).
 * Descriptor  SC [20 rings][60 sectors] f32 per scan.  For every point with finite x, y, z, in float64: r = sqrt(x^2 + y^2),
 *   theta = atan2(y, x) (+ 2 pi if negative); skipped unless r < 80; ring = min(19, floor(r / 4)), sector = min(59, floor(theta /
 *   (2 pi) * 60)), evaluated in that order (a point on the +y, -x or -y axis then opens sector 15, 30, 45); SC[ring][sector] = max over
 *   its points of (float)z + 2.0f; an empty bin is 0.  Further columns of a point are ignored.
 * Prepared    per column c, in f32: norm^2 = fmaf(v_r, v_r, acc) over r = 0..19 in order, norm = its correctly rounded square root,
 *   u[c * 20 + r] = v_r / norm (0 for a zero column), bit c of `valid` = norm > 0.
 * Distance    of query i to candidate j at shift s in 0..59: num_s = the f32 fmaf chain over k = 0..1199 ascending, from 0, of
 *   u_i[k] * u_j[(k + 20 s) mod 1200]; n_s = popcount(valid_i & rot_s(valid_j)), bit c of rot_s = bit (c + s) mod 60 of valid_j;
 *   d_s = 1.0f - num_s / (float)n_s.  A shift with n_s < min_cols, or whose d_s is not below +inf, is skipped.  d(i, j) = min_s d_s, the
 *   lowest s among equals; no shift left: no distance (+inf, shift -1).  If the sensor at frame i is yawed by +psi against frame j at
 *   the same place, s ~ psi / 6 degrees: turning scan i by +s * 6 degrees about z brings it to j's heading.
 * Search      the candidates of query i are j in [0, i - min_gap]; the result is the k <= 8 best by (d, then lower j), with max_dist
 *   (+inf: none) only those with d < max_dist; empty slots are -1 / +inf / -1.
 * caelo_scan_context: pts [n_frames][ld][cols] f32 (cols 3 or 4), n_pts [n_frames] i32 (DEVICE; points 0 .. min(n_pts, ld) - 1 of a frame
 *   count) -> sc [n_frames][20][60] f32, u [n_frames][1200] f32 (16-byte aligned), valid [n_frames] u64.  ws: caelo_sc_ws_bytes(n_frames)
 *   bytes, 16-byte aligned, no initialisation needed.  One fill and two launches on `stream`; nothing waits.  The same input gives the
 *   same bytes on every run.
 * caelo_loop_search: u [n][1200], valid [n] as above; queries [q0, q1) (a running odometry asks for its new frames only) ->
 *   cand, shift [q1 - q0][k] i32, dist [q1 - q0][k] f32; dense_dist [q1 - q0][n] f32 and dense_shift [q1 - q0][n] i8 (both or neither,
 *   +inf / -1 outside the candidates; for tests and evaluation, refused above n = 4096).  ws: caelo_loop_search_ws_bytes(n, q0, q1,
 *   min_gap, k) bytes (0 for arguments that are refused), 16-byte aligned, no initialisation needed.  Two launches; nothing waits; no
 *   atomic decides a result.
 * Refused before any launch (CAELO_ERR_ARG): a null argument (but the dense pair), cols other than 3 or 4, ld outside [1, 2^31), n_frames
 *   outside [0, 65535], n outside [1, 2^24], a query range outside 0 <= q0 <= q1 <= n, k outside 1..8, min_gap < 1, min_cols outside
 *   1..60, a NaN max_dist, one dense output without the other, dense outputs above 4096 frames, a ws or u that is not 16-byte aligned.
 * caelo_host_scan_context, caelo_host_loop_search: the same functions compiled for the host over HOST arrays, with fmaf, sqrtf and / in
 *   the same order; no context, no device. */
int64_t caelo_sc_ws_bytes(int64_t n_frames);
int caelo_scan_context(caelo_ctx *ctx, const float *pts, int64_t ld, int cols, const int32_t *n_pts, int64_t n_frames, float *sc, float *u,
                       uint64_t *valid, void *ws, void *stream);
int caelo_host_scan_context(const float *pts_host, int64_t ld, int cols, const int32_t *n_pts_host, int64_t n_frames, float *sc_host,
                            float *u_host, uint64_t *valid_host);
int64_t caelo_loop_search_ws_bytes(int64_t n, int64_t q0, int64_t q1, int min_gap, int k);
int caelo_loop_search(caelo_ctx *ctx, const float *u, const uint64_t *valid, int64_t n, int64_t q0, int64_t q1, int min_gap, int k,
                      float max_dist, int min_cols, int32_t *cand, float *dist, int32_t *shift, float *dense_dist, int8_t *dense_shift,
                      void *ws, void *stream);
int caelo_host_loop_search(const float *u_host, const uint64_t *valid_host, int64_t n, int64_t q0, int64_t q1, int min_gap, int k,
                           float max_dist, int min_cols, int32_t *cand_host, float *dist_host, int32_t *shift_host, float *dense_dist_host,
                           int8_t *dense_shift_host);

#ifdef __cplusplus
}
#endif
#endif /* CAELO_H */
