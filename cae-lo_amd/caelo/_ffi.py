"""ctypes binding of libcaelo.so (include/caelo.h).  The only place the C ABI is touched.

There is deliberately no fallback: if the shared library is missing or no HIP device exists the
import / context creation fails loudly (the oracle under oracle/ is test infrastructure and is
never reachable from here).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CAELO_LIB") or os.path.join(_HERE, "libcaelo.so")   # CAELO_LIB: A/B runs of a variant build (tools/)

c_vp, c_i64, c_i32, c_int = C.c_void_p, C.c_int64, C.c_int32, C.c_int


class CaeloError(RuntimeError):
    pass


class PoseResult(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("T", C.c_float * 3), ("R_ransac", C.c_float * 9),
                ("T_ransac", C.c_float * 3), ("threshold", C.c_float), ("success", c_i32),
                ("iterations", c_i32), ("n_inliers", c_i32), ("best_trial", c_i32), ("n_pairs", c_i32)]


class IcpParams(C.Structure):
    _fields_ = [("threshold0", C.c_double), ("threshold1", C.c_double), ("decay0", C.c_double), ("decay1", C.c_double),
                ("small_shift", C.c_double), ("ep", C.c_double), ("max_iter", c_i32), ("min_iter", c_i32), ("min_pairs", c_i32),
                ("fail_only_first", c_i32), ("use_planar", c_i32), ("reserved", c_i32)]


class IcpResult(C.Structure):
    _fields_ = [("R_star", C.c_double * 9), ("T_star", C.c_double * 3), ("threshold0", C.c_double), ("threshold1", C.c_double),
                ("iterations", c_i32), ("success", c_i32), ("n_inliers_pts", c_i32), ("n_inliers_planar", c_i32)]


class IssParams(C.Structure):
    """caelo_iss_params (include/caelo.h)."""
    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma_21", C.c_double), ("gamma_32", C.c_double),
                ("min_neighbors", c_i32), ("reserved", c_i32)]


class HarrisParams(C.Structure):
    """caelo_harris_params (include/caelo.h)."""
    _fields_ = [("radius", C.c_double), ("threshold", C.c_double)]


class SiftParams(C.Structure):
    """caelo_sift_params (include/caelo.h)."""
    _fields_ = [("n_scales", c_i32), ("reserved", c_i32), ("min_contrast", C.c_double), ("sigma", C.c_double * 19)]


class FrameJob(C.Structure):
    """caelo_frame_job (include/caelo.h): one frame of the pipeline, device pointers as integers."""
    _fields_ = [("pc", c_vp), ("n", c_i64), ("dist_channels", c_i32), ("mode", c_i32), ("rows", c_vp),
                ("key_pixels", c_vp), ("n_key", c_vp), ("flags", c_vp), ("status", c_vp), ("pair", c_i32),
                ("reserved", c_i32), ("prev_rows", c_vp), ("prev_n_key", c_vp), ("rand", c_vp), ("result", c_vp),
                ("inlier_mask", c_vp), ("pair_idx", c_vp), ("cert", c_vp), ("result_host", c_vp), ("mask_host", c_vp),
                ("rand_host", c_vp), ("info_host", c_vp)]


PAIR_NONE, PAIR_CHAIN, PAIR_EXPLICIT = 0, 1, 2
EXTRACT_EXACT_VOXELS, EXTRACT_NO_DEDUP, EXTRACT_EXACT_PATCHES = 1, 2, 4   # caelo_extract / caelo_frame_job.mode bits (include/caelo.h)
ST_TIES_LEFT = 64   # status bit of the EXTRACT_EXACT_PATCHES mode: a kd build gave up, a tie-split patch kept the canonical rule
EXTRACT_GIVEN_KEYPTS, EXTRACT_GIVEN_ROWS = 8, 16   # the caller's key points (caelo_extract / jobs); the caller's rows (jobs only)
ST_BAD_KEYPTS = 128   # status bit of EXTRACT_GIVEN_KEYPTS: K outside [1, 1024], or a coordinate non-finite or beyond GIVEN_KEYPTS_RANGE
GIVEN_KEYPTS_RANGE = 16384.0   # metres, include/caelo.h CAELO_GIVEN_KEYPTS_RANGE
EXTRACT_CORRECT_PC = 32   # the scan is rotated by the context's calibration angle first (caelo_set_calib_angle; CorrectPC)
ABI_VERSION = 6   # include/caelo.h CAELO_ABI_VERSION
ACT_SIGMOID = 3   # include/caelo.h CAELO_ACT_SIGMOID: the decoder's output activation (caelo_set_decoder_model)
ACT_TANH, ACT_RELU, ACT_LINEAR = 0, 1, 2   # include/caelo.h CAELO_ACT_*: the encoder's activations (caelo_set_encoder_model)
KP_NN_MAX_K, KP_NN_MAX_THRESHOLDS = 65536, 16   # include/caelo.h CAELO_KP_NN_MAX_K / CAELO_KP_NN_MAX_THRESHOLDS (caelo_kp_nn_pairs)
ISS_MAX_POINTS = 32768   # include/caelo.h CAELO_ISS_MAX_POINTS (caelo_iss_keypoints)
SIFT_K, SIFT_MAX_SCALES = 25, 19   # include/caelo.h CAELO_SIFT_K / CAELO_SIFT_MAX_SCALES (caelo_sift_octave)
BUILD_PACKED_F32, BUILD_PROF, BUILD_STAMPED = 1, 2, 256   # caelo_build_flags() bits (include/caelo.h)

# the same layout as a NumPy record (a run's jobs are filled column-wise and handed over in one call)
import numpy as _np
JOB_DTYPE = _np.dtype([("pc", "u8"), ("n", "i8"), ("dist_channels", "i4"), ("mode", "i4"), ("rows", "u8"), ("key_pixels", "u8"),
                       ("n_key", "u8"), ("flags", "u8"), ("status", "u8"), ("pair", "i4"), ("reserved", "i4"), ("prev_rows", "u8"),
                       ("prev_n_key", "u8"), ("rand", "u8"), ("result", "u8"), ("inlier_mask", "u8"), ("pair_idx", "u8"), ("cert", "u8"),
                       ("result_host", "u8"), ("mask_host", "u8"), ("rand_host", "u8"), ("info_host", "u8")], align=True)
assert JOB_DTYPE.itemsize == C.sizeof(FrameJob) and all(JOB_DTYPE.fields[n][1] == getattr(FrameJob, n).offset for n, _ in FrameJob._fields_)
# caelo_ransac_cert (include/caelo.h): what a RANSAC call leaves for the host half (csrc/certify.hip)
CERT_MAX_PAIRS, CERT_MAGIC, CERT_NO_BOUNDS = 1024, 0x43455254, 1
CERT_DTYPE = _np.dtype([("magic", "i4"), ("n_pairs", "i4"), ("flags", "i4"), ("levels_up", "i4"), ("reserved", "i4", (12,)), ("hi", "i4", (512,)),
                        ("idx", "i4", (512, 4)), ("p0", "f4", (CERT_MAX_PAIRS, 3)), ("p1", "f4", (CERT_MAX_PAIRS, 3)),
                        ("hi_up", "i4", (2, 512)), ("idx_up", "i4", (2, 512, 4))])
POSE_DTYPE = _np.dtype([("R", "f4", (9,)), ("T", "f4", (3,)), ("R_ransac", "f4", (9,)), ("T_ransac", "f4", (3,)), ("threshold", "f4"),
                        ("success", "i4"), ("iterations", "i4"), ("n_inliers", "i4"), ("best_trial", "i4"), ("n_pairs", "i4")])
assert POSE_DTYPE.itemsize == C.sizeof(PoseResult)
# caelo_adaptive_result (include/caelo.h): the comparison protocol's registrar (csrc/adaptive.hip)
ADAPTIVE_MAX_TRIALS, ADAPTIVE_DRAWS = 10000, 10001   # include/caelo.h CAELO_ADAPTIVE_MAX_TRIALS / CAELO_ADAPTIVE_DRAWS
ADAPTIVE_DTYPE = _np.dtype([("R", "f8", (9,)), ("T", "f8", (3,)), ("R_ransac", "f8", (9,)), ("T_ransac", "f8", (3,)), ("n_pairs", "i4"),
                            ("n_inliers", "i4"), ("trials", "i4"), ("best_trial", "i4"), ("status", "i4"), ("reserved", "i4")])
assert ADAPTIVE_DTYPE.itemsize == 216
PLANAR_MAX = 48 * 1776   # include/caelo.h CAELO_PLANAR_MAX (caelo_planar_points)
SC_RINGS, SC_SECTORS, LOOP_DENSE_MAX = 20, 60, 4096   # the Scan Context image; caelo_loop_search's dense outputs stop at 4096 frames

# (name, restype, argtypes) -- must list every symbol include/caelo.h declares
SIGNATURES = [
    ("caelo_abi_version", c_int, []),
    ("caelo_build_flags", c_int, []),
    ("caelo_last_error", C.c_char_p, []),
    ("caelo_create", c_int, [C.POINTER(c_vp), c_int]),
    ("caelo_destroy", None, [c_vp]),
    ("caelo_set_respond_weights", c_int, [c_vp] + [c_vp] * 4),
    ("caelo_set_encoder_weights", c_int, [c_vp] + [c_vp] * 10),
    ("caelo_set_encoder_model", c_int, [c_vp] + [c_vp] * 10 + [c_int, c_int]),
    ("caelo_get_encoder_activations", c_int, [c_vp, c_vp]),
    ("caelo_host_encoder_range", c_int, [c_vp] * 10 + [c_int, c_int, c_vp]),
    ("caelo_set_encoder_reference", c_int, [c_vp, c_int]),
    ("caelo_set_decoder_model", c_int, [c_vp] + [c_vp] * 10 + [c_int, c_int]),
    ("caelo_get_decoder_activations", c_int, [c_vp, c_vp]),
    ("caelo_host_decoder_fold", c_int, [c_vp, c_int, c_int, c_vp]),
    ("caelo_decode_ws_bytes", c_i64, [c_i64]),
    ("caelo_decode_ws_layout", c_int, [c_i64, c_vp]),
    ("caelo_decode", c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp, C.c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_train_param_layout", c_int, [c_vp]),
    ("caelo_train_ws_bytes", c_i64, [c_i64]),
    ("caelo_train_ws_layout", c_int, [c_i64, c_vp]),
    ("caelo_autoencoder_grad", c_int, [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_adadelta_step", c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, C.c_float, C.c_float, C.c_float, c_vp]),
    ("caelo_ring_train_param_layout", c_int, [c_vp]),
    ("caelo_ring_train_ws_bytes", c_i64, [c_int, c_int, c_i64]),
    ("caelo_ring_train_ws_layout", c_int, [c_int, c_int, c_i64, c_vp]),
    ("caelo_ring_autoencoder_grad", c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_adam_step", c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, c_vp]),
    ("caelo_correct_pc", c_int, [c_vp, c_vp, c_i64, c_int, C.c_double, c_vp, c_vp]),
    ("caelo_set_calib_angle", c_int, [c_vp, C.c_double]),
    ("caelo_get_calib_angle", C.c_double, [c_vp]),
    ("caelo_project", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_respond", c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    ("caelo_keypoints_ws_bytes", c_i64, []),
    ("caelo_keypoints", c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_debug_read", c_int, [c_vp]),
    ("caelo_voxmap_create", c_int, [c_vp, c_i64, C.POINTER(c_vp)]),
    ("caelo_voxmap_destroy", None, [c_vp]),
    ("caelo_voxelize", c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    ("caelo_voxelize_fast", c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    ("caelo_voxmap_dump", c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_voxmap_counts", c_int, [c_vp, c_vp, c_vp, c_vp]),
    ("caelo_voxmap_export", c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_voxmap_order", c_int, [c_vp, c_vp, c_int, c_vp]),
    ("caelo_voxmap_from_lists", c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_patches", c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_patches_many", c_int, [c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_voxmap_kd_dump", c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_unpack_patches", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_pack_patches", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_encode_ws_bytes", c_i64, [c_i64]),
    ("caelo_encode_ws_layout", c_int, [c_i64, c_vp]),
    ("caelo_encode", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_int, c_vp, c_vp]),
    ("caelo_encode_profile", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    ("caelo_patches32", c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_vp, c_vp, c_vp]),
    ("caelo_set_encoder32_dense", c_int, [c_vp, c_vp, c_vp]),
    ("caelo_encode32_ws_bytes", c_i64, [c_i64]),
    ("caelo_encode32_ws_layout", c_int, [c_i64, c_vp]),
    ("caelo_encode32", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_int, c_vp, c_vp]),
    ("caelo_encode32_profile", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    ("caelo_match_ws_bytes", c_i64, [c_i64]),
    ("caelo_match_ws_bytes_dim", c_i64, [c_i64, c_int]),
    ("caelo_match", c_int, [c_vp, c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_i64, c_vp, c_int, c_vp, c_vp, c_vp]),
    ("caelo_match_profile", c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    ("caelo_solve_rt", c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_ransac_ws_bytes", c_i64, []),
    ("caelo_ransac", c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_cert_bytes", c_i64, []),
    ("caelo_host_bind_blas", c_int, [c_vp, c_vp, c_vp, c_int]),
    ("caelo_host_blas_bound", c_int, []),
    ("caelo_host_unbind_blas", c_int, []),
    ("caelo_host_blas_probe", c_int, [c_int, c_vp, c_vp, c_i64, c_vp]),
    ("caelo_host_bound_violations", c_i64, []),
    ("caelo_host_solve_rt", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    ("caelo_host_ransac", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_host_certify", c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_int]),
    ("caelo_extract_ws_bytes", c_i64, []),
    ("caelo_extract_ws_frame_offset", c_i64, []),
    ("caelo_extract_ws_kp_eligible_offset", c_i64, []),
    ("caelo_extract_ws_ring_offset", c_i64, []),
    ("caelo_extract", c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp,
                              c_vp, c_vp]),
    ("caelo_extend_ws_bytes", c_i64, [c_int, c_int]),
    ("caelo_extend_keypts", c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_icp_ws_bytes", c_i64, [c_i64]),
    ("caelo_icp_step", c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, C.c_double, c_int, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_icp_loop_ws_bytes", c_i64, [c_i64, c_i64]),
    ("caelo_icp", c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, C.POINTER(IcpParams), c_vp, c_vp, c_vp]),
    ("caelo_icp_grid_ws_layout", c_int, [c_i64, c_i64, c_i64, c_i64, c_vp]),
    ("caelo_icp_grid", c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, C.POINTER(IcpParams), c_vp, c_vp, c_vp]),
    ("caelo_pipeline_create", c_int, [c_vp, c_int, c_int, c_i64, C.POINTER(c_vp)]),
    ("caelo_pipeline_destroy", None, [c_vp]),
    ("caelo_pipeline_cert_stats", c_int, [c_vp, C.POINTER(c_i64)]),
    ("caelo_pipeline_batch", c_int, [c_vp]),
    ("caelo_pipeline_begin", c_int, [c_vp, c_vp]),
    ("caelo_pipeline_submit", c_int, [c_vp, C.POINTER(FrameJob)]),
    ("caelo_pipeline_submit_many", c_int, [c_vp, c_vp, c_i64]),
    ("caelo_pipeline_flush", c_int, [c_vp, c_vp]),
    ("caelo_pipeline_wait_encoded", c_int, [c_vp, c_vp]),
    ("caelo_pipeline_sync_encoded", c_int, [c_vp, c_int]),
    ("caelo_pipeline_set_pace", c_int, [c_vp, c_int]),
    ("caelo_pipeline_get_pace", c_int, [c_vp]),
    ("caelo_pipeline_streams", c_int, [c_vp, c_vp]),
    ("caelo_pipeline_extract_ws_read", c_int, [c_vp, c_int, c_i64, c_i64, c_vp, c_vp]),
    ("caelo_upload_many", c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    ("caelo_pipeline_run_uploading", c_int, [c_vp, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_i64, c_int, c_vp, c_vp, c_vp]),
    ("caelo_host_random_sample", c_int, [C.c_uint32, c_i64, c_vp]),
    ("caelo_seqloader_slot_bytes", c_i64, [c_int, c_i64]),
    ("caelo_seqloader_create", c_int, [c_vp, c_i64, c_i64, c_int, c_int, c_i64, c_vp, c_vp, c_int, c_i64, c_int, c_vp]),
    ("caelo_seqloader_wait", c_int, [c_vp, c_i64, c_vp, c_vp]),
    ("caelo_seqloader_release", c_int, [c_vp, c_i64]),
    ("caelo_seqloader_stats", c_int, [c_vp, c_vp]),
    ("caelo_seqloader_destroy", None, [c_vp]),
    ("caelo_pipeline_stats", c_int, [c_vp, C.POINTER(c_i64)]),
    ("caelo_pipeline_expect", c_int, [c_vp, c_i64]),
    ("caelo_lane_faults", c_int, [c_vp, C.POINTER(c_i64)]),
    ("caelo_kp_nn_pairs", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_vp, c_vp]),
    ("caelo_iss_ws_bytes", c_i64, [c_i64, c_int]),
    ("caelo_iss_keypoints", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, C.POINTER(IssParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    ("caelo_harris_ws_bytes", c_i64, [c_i64, c_int]),
    ("caelo_harris_keypoints", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, C.POINTER(HarrisParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    ("caelo_sift_ws_bytes", c_i64, [c_i64, c_int]),
    ("caelo_sift_octave", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, C.POINTER(SiftParams), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    ("caelo_voxel_centroids", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp]),
    ("caelo_register_pairs_ws_bytes", c_i64, [c_i64]),
    ("caelo_register_pairs", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_register_pairs_ws_bytes_dim", c_i64, [c_i64, c_int]),
    ("caelo_register_pairs_desc", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int]),
    ("caelo_ransac_adaptive", c_int, [c_vp, c_vp, c_vp, c_i64, c_vp, C.c_double, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_host_ransac_adaptive", c_int, [c_vp, c_vp, c_i64, c_vp, C.c_double, c_vp, c_vp]),
    ("caelo_register_pairs_adaptive_ws_bytes", c_i64, [c_i64, c_int]),
    ("caelo_register_pairs_adaptive", c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, C.c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int]),
    ("caelo_planar_ws_bytes", c_i64, []),
    ("caelo_planar_points", c_int, [c_vp, c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_host_planar_points", c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_sc_ws_bytes", c_i64, [c_i64]),
    ("caelo_scan_context", c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_host_scan_context", c_int, [c_vp, c_i64, c_int, c_vp, c_i64, c_vp, c_vp, c_vp]),
    ("caelo_loop_search_ws_bytes", c_i64, [c_i64, c_i64, c_i64, c_int, c_int]),
    ("caelo_loop_search", c_int, [c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_int, c_int, C.c_float, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    ("caelo_host_loop_search", c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_int, c_int, C.c_float, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
]

_lib = None


def load():
    """dlopen libcaelo.so and type every entry point.  Raises if the library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CaeloError("libcaelo.so not built (%s); run `python __graft_entry__.py` or "
                             "`make -C cae-lo_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
        # torch bundles its own HIP runtime: load it first so libcaelo.so binds to the same libamdhip64
        # (two runtimes in one process cannot both own the device)
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.caelo_abi_version() != ABI_VERSION:
            raise CaeloError("libcaelo.so ABI mismatch")
        if lib.caelo_cert_bytes() != CERT_DTYPE.itemsize:
            raise CaeloError("caelo_ransac_cert layout mismatch")
        word = lib.caelo_build_flags()
        if not word & BUILD_STAMPED or (word & BUILD_PACKED_F32 and not os.environ.get("CAELO_ALLOW_PACKED_F32")):
            # packed-f32 VALU ops drop an operand in lanes 48-63 under three busy queues on MI355X: such a
            # binary gives a wrong pose about once in 1 000 frames.  tools/stress_pairs.py sets CAELO_ALLOW_PACKED_F32 to
            # demonstrate exactly that; nothing else may.
            raise CaeloError("%s was not built by csrc/Makefile with -packed-fp32-ops (build word %d); refusing to load it"
                             % (LIB_PATH, word))
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise CaeloError("libcaelo error %d: %s" % (rc, load().caelo_last_error().decode()))
