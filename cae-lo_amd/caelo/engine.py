"""Device engine: one HIP context + weights + reusable buffers per process (one process per GPU).

``Engine`` owns the libcaelo context, loads the two Keras ``.h5`` files through ``h5lite`` and
exposes (a) stage methods on device tensors, one per C-ABI entry point, and (b) the fused hot
path ``extract`` (scan -> keypoints + 60-d descriptors) and ``match_pose`` (two frames -> rigid
pose) that run without any host synchronisation until the caller reads a result.

PyTorch is used for device memory and streams only.
"""
import collections
import ctypes as C
import os
import threading
import time

import numpy as np
import torch

from . import _ffi
from .h5lite import H5File

RING_H, RING_W, RING_C = 69, 1800, 5
NET_H, NET_W = 64, 1792
MAX_K = 1024

ST_COL_OOB, ST_VOXEL_OOB, ST_MAP_FULL, ST_FEW_VOXELS, ST_FEW_KEYPTS, ST_NONFINITE = 1, 2, 4, 8, 16, 32
ST_TIES_LEFT = _ffi.ST_TIES_LEFT   # not an error: the exact_patches mode left a tie-split patch on the canonical rule
ST_BAD_KEYPTS = _ffi.ST_BAD_KEYPTS   # given key points (extract(key_pts=...), Pipeline.run(keypts=...)) the engine cannot serve

_DEFAULT_WEIGHTS = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "weights")
RESPOND_H5 = os.path.join(_DEFAULT_WEIGHTS, "SphericalRingPCRespondLayer.h5")
ENCODER_H5 = os.path.join(_DEFAULT_WEIGHTS, "EncoderModel4VoxelPatch.h5")


# Keras layouts of the two networks' weights, kernel then bias per layer (Engine.set_encoder_weights / set_respond_weights)
ENCODER_SHAPES = [(3, 3, 3, 1, 8), (8,), (3, 3, 3, 8, 16), (16,), (3, 3, 3, 16, 32), (32,), (2048, 200), (200,), (200, 20), (20,)]
RESPOND_SHAPES = [(3, 3, 3, 32), (32,), (1, 1, 32, 8), (8,)]
# the decoder half of an autoencoder file: dense_3, dense_4, conv3d_4 .. conv3d_6 (Engine.set_decoder_weights)
DECODER_SHAPES = [(20, 200), (200,), (200, 2048), (2048,), (3, 3, 3, 32, 16), (16,), (3, 3, 3, 16, 8), (8,), (3, 3, 3, 8, 1), (1,)]


IssKeypoints = collections.namedtuple("IssKeypoints", "key_idx n_key saliency eig n_neigh")   # Engine.iss_keypoints
HarrisKeypoints = collections.namedtuple("HarrisKeypoints", "key_idx n_key response n_neigh normals")   # Engine.harris_keypoints
SiftOctave = collections.namedtuple("SiftOctave", "key_idx n_key dog knn key_mask")   # Engine.sift_octave
SiftKeypoints = collections.namedtuple("SiftKeypoints", "xyz scale octave n_key")   # Engine.sift_keypoints


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _hptr(a):
    return a.ctypes.data_as(C.c_void_p)


def raise_status(st):
    """Map device status bits to the exception the reference would raise (SURVEY 8b 'Errors')."""
    if st & ST_BAD_KEYPTS:   # (a deviation: the reference raises nothing there -- include/caelo.h CAELO_ST_BAD_KEYPTS)
        raise ValueError("given key points: K must lie in [1, %d] and every coordinate must be finite with |x|, |y|, |z| <= %g m"
                         % (MAX_K, _ffi.GIVEN_KEYPTS_RANGE))
    if st & ST_COL_OOB:
        raise IndexError("index 1800 is out of bounds for axis 1 with size 1800")  # SphericalRing.py:91
    if st & ST_VOXEL_OOB:
        raise IndexError("voxel index out of bounds for axis with size 64")        # Voxel.py:139
    if st & ST_NONFINITE:
        raise ValueError("cannot convert float NaN to integer")                    # SphericalRing.py:86-88, Voxel.py:122-124
    if st & ST_FEW_VOXELS:
        raise ValueError("Expected n_neighbors <= n_samples (n_neighbors = 496)")  # Voxel.py:195-196
    if st & ST_FEW_KEYPTS:
        raise AssertionError("KeyPts.shape[0] > 50")                               # SphericalRing.py:286
    if st & ST_MAP_FULL:
        raise _ffi.CaeloError("voxel map overflow")


def extract_mode(exact_voxels=False, dedup=True, exact_patches=False, given_keypts=False, given_rows=False, correct_pc=False):
    """The CAELO_EXTRACT_* mode word of caelo_extract / caelo_frame_job."""
    if given_rows:
        return _ffi.EXTRACT_GIVEN_ROWS
    return ((_ffi.EXTRACT_EXACT_VOXELS if exact_voxels else 0) | (0 if dedup else _ffi.EXTRACT_NO_DEDUP)
            | (_ffi.EXTRACT_EXACT_PATCHES if exact_patches else 0) | (_ffi.EXTRACT_GIVEN_KEYPTS if given_keypts else 0)
            | (_ffi.EXTRACT_CORRECT_PC if correct_pc else 0))


def _given_pts(eng, key_pts):
    """A caller's key points as a [K,3] f32 tensor on the engine's device (K is checked on the device: CAELO_ST_BAD_KEYPTS)."""
    t = key_pts if isinstance(key_pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(key_pts, dtype=np.float32))
    t = t.to(device=eng.device, dtype=torch.float32)
    assert t.dim() == 2 and t.shape[1] == 3, "key points: [K, 3]"
    return t


def note_ties_left(eng, st):
    """Status word(s) already read by the caller: where CAELO_ST_TIES_LEFT is set (exact_patches mode: a kd build gave up, a tie-split
    patch kept the canonical rule and flags & 2), record it in ``eng.last_tie_unresolved`` and warn, like ``Engine.resolve_ties_many``.
    -> number of frames concerned."""
    n = int(np.count_nonzero(np.asarray(st) & ST_TIES_LEFT))
    if n:
        eng.last_tie_unresolved = n
        import warnings
        warnings.warn("%d frame(s) kept tie-split patch(es) on the canonical rule: the kd-tree redo gave up (flags & 2 still set)" % n)
    return n


ACTIVATION_CODES = {"tanh": _ffi.ACT_TANH, "relu": _ffi.ACT_RELU, "linear": _ffi.ACT_LINEAR}
ACTIVATION_NAMES = {v: k for k, v in ACTIVATION_CODES.items()}
ACTIVATION_NAMES[_ffi.ACT_SIGMOID] = "sigmoid"   # the decoder's output only (caelo_set_decoder_model)
# Engine.decode's result: the tensors that were asked for, None for the others
Decoded = collections.namedtuple("Decoded", "prob bits loss counts")
ENCODER_LAYERS = ("conv3d_1", "conv3d_2", "conv3d_3", "dense_1", "dense_2")   # caelo_host_encoder_range's five bounds, in order


def _activation_codes(activations):
    """("relu", "linear") or CAELO_ACT_* integers -> (hidden, code) as CAELO_ACT_* integers; ValueError for anything else."""
    try:
        h, c = activations
        h, c = (ACTIVATION_CODES[a] if isinstance(a, str) else int(a) for a in (h, c))
    except (KeyError, TypeError, ValueError):
        raise ValueError("encoder activations: (hidden, code) with hidden in ('tanh', 'relu') and code in ('tanh', 'linear'), got %r" % (activations,))
    if h not in (_ffi.ACT_TANH, _ffi.ACT_RELU) or c not in (_ffi.ACT_TANH, _ffi.ACT_LINEAR):
        raise ValueError("encoder activations: (hidden, code) with hidden in ('tanh', 'relu') and code in ('tanh', 'linear'), got %r" % (activations,))
    return h, c


def read_keras_model(path):
    """-> ("respond", [w1,b1,w2,b2], None) or ("encoder", [10 arrays], (H, C)) from a Keras 2.2 .h5 file: keras_config.read_model."""
    from . import keras_config
    return keras_config.read_model(path)


def read_keras_weights(path):
    """-> ("respond", [w1,b1,w2,b2]) or ("encoder", [10 arrays]): read_keras_model without the activations."""
    return read_keras_model(path)[:2]


class VoxelMap:
    def __init__(self, eng, max_points):
        self.eng, self.max_points = eng, int(max_points)
        h = C.c_void_p()
        _ffi.check(eng.lib.caelo_voxmap_create(eng.ctx, self.max_points, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                self.eng.lib.caelo_voxmap_destroy(self.h)
                self.h = None
        except Exception:
            pass


class FrameFeatures:
    """Device-resident result of Engine.extract for one scan.  ``rows`` [1024,64] f32 holds the
    60-d descriptor (cols 0:60, 16-byte aligned rows for the match kernel's vector loads) | xyz (60:63)
    | valid flag (63): the unit the multi-GPU all-gather moves; key_pts / features are strided views."""
    __slots__ = ("rows", "key_pts", "key_pixels", "features", "n_key", "status", "flags")

    def __init__(self, rows, key_pixels, n_key, status, flags):
        self.rows = rows
        self.key_pts, self.features = rows[:, 60:63], rows[:, 0:60]
        self.key_pixels, self.n_key, self.status, self.flags = key_pixels, n_key, status, flags

    @classmethod
    def from_rows(cls, rows):
        """Rebuild from gathered rows (another rank's frame): n_key = number of valid rows."""
        n_key = rows[:, 63].sum().round().to(torch.int32).reshape(1)
        return cls(rows, None, n_key, None, None)


class FrameBatch:
    """Device-resident outputs of Pipeline.run for K frames (one allocation per field)."""

    def __init__(self, eng, k):
        self.k = k
        self.rows = eng.empty((k, MAX_K, 64), torch.float32)       # the multi-GPU all-gather payload
        self.key_pixels = eng.empty((k, MAX_K, 2), torch.int64)
        self.n_key = eng.empty((k,), torch.int32)
        self.flags = eng.empty((k, MAX_K, 3), torch.uint8)
        self.status = eng.empty((k, 4), torch.int32)
        self.result = eng.zeros((k, C.sizeof(_ffi.PoseResult)), torch.uint8)   # pair (i-1, i) in slot i
        self.inlier_mask = eng.zeros((k, MAX_K), torch.uint8)
        self.pair_idx = eng.zeros((k, MAX_K), torch.int64)
        self.cert = None       # [k, sizeof(caelo_ransac_cert)] u8 once a run asked for certificates (Pipeline.run(certify=True))
        self.exact = None      # host copy of the certified results: (results [k], masks [k,1024], evals [k], status [k])
        self._rands_host = None
        self._exact_buf = None

    def ensure_cert(self, eng):
        if self.cert is None:
            self.cert = eng.zeros((self.k, _ffi.CERT_DTYPE.itemsize), torch.uint8)
        return self.cert

    def frame(self, i):
        return FrameFeatures(self.rows[i], self.key_pixels[i], self.n_key[i:i + 1], self.status[i], self.flags[i])

    def view(self, start, n):
        """Frames start .. start + n as a FrameBatch over the same storage."""
        v = object.__new__(FrameBatch)
        v.k = n
        for f in ("rows", "key_pixels", "n_key", "flags", "status", "result", "inlier_mask", "pair_idx"):
            setattr(v, f, getattr(self, f)[start:start + n])
        v.cert = self.cert[start:start + n] if self.cert is not None else None
        v.exact = None if self.exact is None else tuple(a[start:start + n] for a in self.exact)
        v._rands_host = None
        v._exact_buf = None
        return v


class Pipeline:
    """caelo_pipeline (include/caelo.h): `batch` consecutive frames share one launch of every front kernel, one
    encoder launch set and one match / RANSAC launch; the three stages of successive batches overlap on three HIP
    streams.  ``run`` submits K scans and returns without waiting for the GPU."""

    def __init__(self, eng, batch=4, buffers=3, max_points=None):
        self.eng = eng
        h = C.c_void_p()
        _ffi.check(eng.lib.caelo_pipeline_create(eng.ctx, int(batch), int(buffers), int(max_points or eng.max_points), C.byref(h)))
        self.h, self.batch, self.buffers = h, int(batch), int(buffers)
        self.pace = int(eng.lib.caelo_pipeline_get_pace(h))   # the library's default until set_pace (asked, not re-derived from the environment)
        self._slots = None   # the upload modes' device slots: ((count, bytes), tensors)
        self._copy = None    # ... and their copy stream (both made by the first upload call)

    def __del__(self):
        try:
            if self.h:
                self.eng.lib.caelo_pipeline_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def stats(self):
        """Host-side counters since the last call: jobs, us/frame the calling thread spent issuing launches, batches."""
        out = (C.c_int64 * 6)()
        _ffi.check(self.eng.lib.caelo_pipeline_stats(self.h, out))
        n = max(int(out[0]), 1)
        return {"jobs": int(out[0]), "issue_us_per_frame": out[1] / n / 1e3, "batches": int(out[2]), "batch": int(out[3]),
                "buffers": int(out[4]), "streams": int(out[5])}

    def streams(self):
        """caelo_pipeline_streams: the HIP stream handles (ints) of the stages -> {"front", "encoder", "pair", "voxel"}; stages that
        share a stream report the same handle, "voxel" is None when the voxel maps are built on the front stream."""
        out = (C.c_void_p * 4)()
        _ffi.check(self.eng.lib.caelo_pipeline_streams(self.h, out))
        return dict(zip(("front", "encoder", "pair", "voxel"), (out[i] for i in range(4))))

    def extract_ring_and_map(self, i):
        """Test aid: what the last batch left in the extract workspace of its frame ``i`` (caelo_pipeline_extract_ws_read) -> host
        arrays (ring image [69,1800,5] f32, eligibility map [64] uint64, as ``Engine.extract_kp_eligible``).  On the current stream,
        which ``run`` left waiting for every stage; synchronises."""
        eng = self.eng
        out = []
        for off, n in ((int(eng.lib.caelo_extract_ws_ring_offset()), RING_H * RING_W * RING_C * 4),
                       (int(eng.lib.caelo_extract_ws_kp_eligible_offset()), NET_H * 8)):
            buf = eng.empty((n,), torch.uint8)
            _ffi.check(eng.lib.caelo_pipeline_extract_ws_read(self.h, int(i), off, n, _ptr(buf), eng.stream))
            out.append(buf)
        torch.cuda.current_stream(eng.device).synchronize()
        return (out[0].cpu().numpy().view(np.float32).reshape(RING_H, RING_W, RING_C).copy(), out[1].cpu().numpy().view(np.uint64).copy())

    def _jobs(self, ptrs, counts, rands, prev, out, pairs, dist_channels, exact_voxels, dedup, certify=False, rands_host=None, exact_patches=False,
              calib_angle=None):
        """The run's jobs as one record array, filled column-wise, handed over in ONE foreign call (a ctypes call per frame
        costs ~10 us: 380 us for a 20-frame run, most of it before the first launch)."""
        k = len(ptrs)
        jobs = np.zeros(k, dtype=_ffi.JOB_DTYPE)
        idx = np.arange(k, dtype=np.uint64)
        jobs["pc"], jobs["n"] = ptrs, counts
        jobs["dist_channels"], jobs["mode"] = int(dist_channels), extract_mode(exact_voxels, dedup, exact_patches)
        if calib_angle is not None:   # the scans are corrected on the device first (CAELO_EXTRACT_CORRECT_PC, the context's angle)
            jobs["mode"] |= np.where(self.eng._calib_frames(calib_angle, k), _ffi.EXTRACT_CORRECT_PC, 0).astype(np.int32)
        jobs["rows"] = out.rows.data_ptr() + idx * (MAX_K * 256)
        jobs["key_pixels"] = out.key_pixels.data_ptr() + idx * (MAX_K * 16)
        jobs["n_key"] = out.n_key.data_ptr() + idx * 4
        jobs["flags"] = out.flags.data_ptr() + idx * (MAX_K * 3)
        jobs["status"] = out.status.data_ptr() + idx * 16
        if pairs and k > 0:
            jobs["pair"] = _ffi.PAIR_CHAIN
            if prev is not None:
                assert prev.rows.is_contiguous()
                jobs["pair"][0], jobs["prev_rows"][0] = _ffi.PAIR_EXPLICIT, prev.rows.data_ptr()
                jobs["prev_n_key"][0] = prev.n_key.data_ptr() if prev.n_key is not None else 0
            else:
                jobs["pair"][0] = _ffi.PAIR_NONE
            jobs["rand"] = rands[:k] if isinstance(rands, np.ndarray) else [rands[i].data_ptr() for i in range(k)]   # (an array: device addresses)
        else:
            jobs["pair"] = _ffi.PAIR_NONE
        jobs["result"] = out.result.data_ptr() + idx * out.result.shape[1]
        jobs["inlier_mask"] = out.inlier_mask.data_ptr() + idx * MAX_K
        jobs["pair_idx"] = out.pair_idx.data_ptr() + idx * (MAX_K * 8)
        if certify and pairs and k > 0:
            # the exact RANSAC: certificates on the device, and (certify = "host", the default meaning of True) the pipeline's
            # certifier thread writes the exact results to host arrays while later batches run (include/caelo.h)
            self.eng.host_blas()
            if certify == "device" or os.environ.get("CAELO_CERT_ZEROCOPY") == "0":
                jobs["cert"] = out.ensure_cert(self.eng).data_ptr() + idx * _ffi.CERT_DTYPE.itemsize
            if certify != "device":   # (the kernels write these pairs' certificates straight into the pipeline's pinned host memory)
                if out._exact_buf is None:   # host arrays of the exact results: allocated once per FrameBatch
                    out._exact_buf = (np.zeros(out.k, dtype=_ffi.POSE_DTYPE), np.zeros((out.k, MAX_K), dtype=np.uint8),
                                      np.zeros((out.k, 2), dtype=np.int32))
                res, masks, info = out._exact_buf
                info[:k, 0] = 0
                info[:k, 1] = 3                                  # "no record" until the certifier says otherwise
                has = jobs["pair"] != _ffi.PAIR_NONE
                out._has_pair = np.zeros(out.k, dtype=bool)
                out._has_pair[:k] = has
                jobs["result_host"] = np.where(has, res.ctypes.data + idx * _ffi.POSE_DTYPE.itemsize, 0)
                jobs["mask_host"] = np.where(has, masks.ctypes.data + idx * MAX_K, 0)
                jobs["info_host"] = np.where(has, info.ctypes.data + idx * 8, 0)
                if isinstance(rands_host, np.ndarray) and rands_host.dtype == np.uint64:   # host ADDRESSES of the draws (Pipeline.run_loaded: the loader's ring)
                    jobs["rand_host"] = rands_host[:k]
                elif rands_host is not None:   # (float64, contiguous, >= 6000 draws each: checked once per distinct array)
                    seen = {}
                    ptrs = np.empty(k, dtype=np.uint64)
                    for i in range(k):
                        r = rands_host[i]
                        a = seen.get(id(r))
                        if a is None:
                            assert isinstance(r, np.ndarray) and r.dtype == np.float64 and r.flags["C_CONTIGUOUS"] and r.size >= 6000
                            a = seen[id(r)] = r.ctypes.data
                        ptrs[i] = a
                    jobs["rand_host"] = ptrs
                    out._rands_host = rands_host
                out.exact = (res, masks, info[:, 0], info[:, 1])
        return jobs

    def wait_encoded(self, stream):
        """caelo_pipeline_wait_encoded: ``stream`` (a torch stream) waits for the rows of every frame of the batches issued so far."""
        _ffi.check(self.eng.lib.caelo_pipeline_wait_encoded(self.h, C.c_void_p(stream.cuda_stream)))

    def sync_encoded(self, lag=0):
        """caelo_pipeline_sync_encoded: the calling thread waits until the rows of every batch issued so far, except the last
        ``lag``, are written (no device-side wait is left in any queue)."""
        _ffi.check(self.eng.lib.caelo_pipeline_sync_encoded(self.h, int(lag)))

    def run(self, scans, rands=None, prev=None, dist_channels=5, exact_voxels=False, out=None, pairs=True, dedup=True, on_batch=None,
            on_encoded=None, certify=False, rands_host=None, publish=True, exact_patches=False, keypts=None, rows_given=None, calib_angle=None):
        """scans: K device tensors [n,4] f32; rands: K device tensors of RANSAC draws ([1500,4] f64).
        Frame i is matched against frame i-1 (pose in ``result[i]``); frame 0 against ``prev``
        (FrameFeatures) when given; ``pairs=False`` extracts only (BASELINE configs[1]).  Returns a FrameBatch; the
        current stream has waited for all lanes.  ``certify=True``: the exact RANSAC -- every pair leaves its certificate
        (``out.cert``) and the pipeline's certifier thread runs the host half (csrc/certify.hip) on it while later batches are on
        the GPU; when ``run`` returns, ``out.exact`` = (results record array [k], masks [k,1024] u8, evals [k], status [k]) holds
        the reference's inlier sets, R_star / T_star and refits bit for bit (frames without a pair: status 3) and
        ``out.result`` / ``out.inlier_mask`` on the device are overwritten with them.  ``rands_host``: host copies of the draws
        (only read for a pair that escalates beyond 0.4 m; fetched from the device otherwise).  ``certify="device"``: certificates
        only (``Engine.certify_batch`` runs the host half later).  ``publish=False``: the exact results stay in ``out.exact`` (host
        arrays, where the reference's own results live) and ``out.result`` / ``out.inlier_mask`` on the device are NOT written at all
        (with the host half active the kernels stop at the certificate: no k_ransac_finish).  ``on_encoded(lo, hi)`` is called, in order, once the rows of frames [lo, hi) are
        WRITTEN (the calling thread has waited for them: caelo_pipeline_sync_encoded, one batch behind the issue) -- what it
        enqueues on any stream may read them at once; a caller ships finished rows that way while later batches run.
        ``on_batch(lo, hi)`` is called right after frames [lo, hi) have been issued (with ``wait_encoded`` the device-side form of
        the same hand-over, which costs the pipeline a quarter of its rate: DESIGN.md 6).  ``exact_patches=True``: the reference's
        patches (caelo_extract's CAELO_EXTRACT_EXACT_PATCHES) -- tie-split patches are redone on the device inside the run, so the
        descriptors, matches and RANSAC results are the reference's with no host redo; ``out.status`` may carry ST_TIES_LEFT.
        Other key point sources, per frame (a frame with neither uses the detector, so runs may mix them; the pipeline splits a batch
        where the kind changes, pairs chain across): ``keypts[i]`` = [K,3] f32 key points of frame i (CAELO_EXTRACT_GIVEN_KEYPTS, see
        ``Engine.extract``); ``rows_given[i]`` = [K,64] f32 rows (descriptor zero-padded to columns 0:60 | xyz 60:63 | valid 63,
        ``keysources.rows_from_features``) that are matched as they are (CAELO_EXTRACT_GIVEN_ROWS, isLoadFeaturesFromFile): no scan
        needed (``scans[i]`` may be None), ``out.status[i]`` / ``flags[i]`` are zero and ``key_pixels[i]`` -1.
        ``calib_angle``: degrees; every scan is first corrected by the reference's CorrectPC on the device (``Engine.extract``), one
        launch per batch at the head of the front stage; the caller's scans are not written.  A sequence with one entry per frame
        (the angle, or None for a frame that is not corrected) mixes both kinds: a batch is split where the kind changes.  Given key
        points and given rows are never corrected (the reference corrects scans only)."""
        eng, lib, k = self.eng, self.eng.lib, len(scans)
        out = out or FrameBatch(eng, k)
        assert out.k >= k and (not pairs or len(rands) >= k)
        stream = eng.stream
        modes = self._given(out, k, keypts, rows_given)
        per_batch = on_batch is not None or on_encoded is not None
        # an even batch plan for runs that are not whole batches (caelo.h); with a per-batch callback: full batches, remainder last
        _ffi.check(lib.caelo_pipeline_expect(self.h, 0 if per_batch else k))
        _ffi.check(lib.caelo_pipeline_begin(self.h, stream))
        for i, pc in enumerate(scans):
            if pc is None and modes is not None and modes[i] == 2:
                continue
            assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] == 4 and pc.is_contiguous()
        _t0 = time.perf_counter()
        jobs = self._jobs([0 if pc is None else pc.data_ptr() for pc in scans], [0 if pc is None else pc.shape[0] for pc in scans], rands,
                          prev, out, pairs, dist_channels, exact_voxels, dedup, certify, rands_host, exact_patches, calib_angle)
        if modes is not None:
            jobs["mode"] = np.where(modes == 1, jobs["mode"] | _ffi.EXTRACT_GIVEN_KEYPTS, np.where(modes == 2, _ffi.EXTRACT_GIVEN_ROWS, jobs["mode"]))
        _t1 = time.perf_counter()
        tail = None   # a partial last batch is only issued by the flush: its callbacks come after that
        issued = []   # batches issued, not yet reported to on_encoded
        try:
            if not per_batch:
                _ffi.check(lib.caelo_pipeline_submit_many(self.h, jobs.ctypes.data, k))
            else:
                for lo in range(0, k, self.batch):
                    hi = min(k, lo + self.batch)
                    _ffi.check(lib.caelo_pipeline_submit_many(self.h, jobs[lo:hi].ctypes.data, hi - lo))
                    if hi - lo == self.batch:
                        if on_batch:
                            on_batch(lo, hi)
                        issued.append((lo, hi))
                        if on_encoded and len(issued) > 1:
                            self.sync_encoded(1)      # (returns at once under the default pacing of the issue)
                            while len(issued) > 1:
                                on_encoded(*issued.pop(0))
                    else:
                        tail = (lo, hi)
        finally:
            rc = lib.caelo_pipeline_flush(self.h, stream)
        _ffi.check(rc)
        if tail:
            if on_batch:
                on_batch(*tail)
            issued.append(tail)
        if on_encoded and issued:
            self.sync_encoded(0)
            for lo, hi in issued:
                on_encoded(lo, hi)
        _t2 = time.perf_counter()
        self._finish_exact(out, k, certify, pairs, publish)
        self.last_times = {"jobs_ms": 1e3 * (_t1 - _t0), "submit_flush_ms": 1e3 * (_t2 - _t1), "publish_ms": 1e3 * (time.perf_counter() - _t2)}
        return out

    def _given(self, out, k, keypts, rows_given):
        """Pipeline.run's other key point sources: their inputs written into ``out`` (on the current stream, which the pipeline's
        stages wait for) -> per-frame kind [k] (0 detector, 1 given key points, 2 given rows), or None when every frame uses the detector."""
        if keypts is None and rows_given is None:
            return None
        modes = np.zeros(k, dtype=np.int32)
        counts = np.zeros(k, dtype=np.int32)
        for i in range(k):
            kp = keypts[i] if keypts is not None else None
            rw = rows_given[i] if rows_given is not None else None
            assert kp is None or rw is None, "frame %d: key points and rows given" % i
            if kp is not None:
                t = _given_pts(self.eng, kp)
                out.rows[i, :min(t.shape[0], MAX_K), 60:63] = t[:MAX_K]
                modes[i], counts[i] = 1, t.shape[0]
            elif rw is not None:
                t = rw if isinstance(rw, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rw, dtype=np.float32))
                assert t.dim() == 2 and t.shape[1] == 64 and 1 <= t.shape[0] <= MAX_K, "given rows: [K, 64] with K in [1, 1024]"
                out.rows[i].zero_()
                out.rows[i, :t.shape[0]] = t.to(device=self.eng.device, dtype=torch.float32)
                out.status[i].zero_()
                out.flags[i].zero_()
                out.key_pixels[i].fill_(-1)
                modes[i], counts[i] = 2, t.shape[0]
        if modes.any():   # (one copy for all the counts; the detector's frames get theirs from the device)
            sel = torch.from_numpy(np.nonzero(modes)[0]).to(self.eng.device)
            out.n_key[:k].index_copy_(0, sel, torch.from_numpy(counts[modes != 0]).to(self.eng.device))
        return modes

    def _finish_exact(self, out, k, certify, pairs, publish=True):
        """After the flush of a certified run: the certifier thread has written every exact result (caelo_pipeline_flush waits
        for it).  Check that every pair came back exact; with ``publish``, put the results into the device tensors too (without,
        they stay in ``out.exact``, where the caller reads them).  Host arrays only: no device read."""
        if not (certify and certify != "device" and pairs and k > 0):
            return
        res, masks, evals, status = out.exact
        if (status[:k] == 2).any():
            raise _ffi.CaeloError("a pair holds more than 1024 matches: no certificate")
        has = getattr(out, "_has_pair", None)
        if has is not None and (status[:k][has[:k]] != 0).any():   # (the flush reports it too: a job WITH a pair must come back exact)
            bad = np.flatnonzero(has[:k] & (status[:k] != 0))
            raise _ffi.CaeloError("pairs of frames %s came back without an exact result (status %s)" % (bad.tolist(), status[:k][bad].tolist()))
        if not publish:
            return
        ok = status[:k] == 0
        if ok.any():
            with torch.cuda.stream(torch.cuda.current_stream(self.eng.device)):
                if ok.all():
                    out.result[:k].copy_(torch.from_numpy(res[:k].view(np.uint8).reshape(k, -1)))
                    out.inlier_mask[:k].copy_(torch.from_numpy(masks[:k]))
                else:
                    sel = torch.from_numpy(np.flatnonzero(ok)).to(self.eng.device)
                    out.result[sel] = torch.from_numpy(np.ascontiguousarray(res[:k].view(np.uint8).reshape(k, -1)[ok])).to(self.eng.device)
                    out.inlier_mask[sel] = torch.from_numpy(np.ascontiguousarray(masks[:k][ok])).to(self.eng.device)

    def cert_stats(self):
        """Host half inside the pipeline since the last call: pairs certified, hypotheses evaluated per pair, certifier-thread us per pair."""
        o = (C.c_int64 * 4)()
        _ffi.check(self.eng.lib.caelo_pipeline_cert_stats(self.h, o))
        n = max(int(o[0]), 1)
        return {"pairs": int(o[0]), "evals_per_pair": o[1] / n, "host_us_per_pair": o[2] / n / 1e3, "handover_us_per_pair": o[3] / n / 1e3}

    def set_pace(self, lag):
        """caelo_pipeline_set_pace: after issuing a batch the calling thread waits for the encoder of the batch ``lag`` before it
        (-1: never)."""
        _ffi.check(self.eng.lib.caelo_pipeline_set_pace(self.h, int(lag)))
        self.pace = int(lag)

    def run_uploading(self, host_scans, rands=None, prev=None, dist_channels=5, out=None, pairs=True, dedup=True, ahead=4, certify=False,
                      rands_host=None, exact_patches=False, calib_angle=None):
        """``run`` for scans that live in (pinned) HOST memory: a copy stream uploads batch b + ``ahead`` while the pipeline works on
        batch b, into ``ahead + 2`` sets of device buffers -- the overlap of the reference's producer process, which prepares
        frame i + 1 while frame i is matched (PoseEstimation.py:214-245).  The loop runs natively (caelo_pipeline_run_uploading) and
        paces the hand-overs from the calling thread, not by waits in the device queues: per batch it waits for the arrival of the
        batch's scans (an event on the copy stream), issues the launches, then the copies of the batch ``ahead`` further on, then waits
        for the encoder of the batch before (caelo_pipeline_sync_encoded: the GPU keeps one batch queued).  The slot the next copy
        overwrites held batch b - 2, whose scans only its front stage read: the wait for the encoder of b - 2 (one iteration earlier)
        covers it; the first ``ahead`` copies of a call wait on the device for the previous call's work (the copy stream waits the
        call's begin, once).  ``ahead``: 13.5 / 15.3 / 15.9 / 16.1 k frames/s for
        1 / 2 / 3 / 4 (18.6 k resident; an arrival is late by up to 0.3 ms now and then, and a batch of scans is 17 MB of device
        memory).  Device-side waits for the same hand-overs cost 8 - 15 % of the resident rate EACH, however rarely they were issued
        (DESIGN.md 5).  Scans of a batch that are views of ONE pinned block at a fixed pitch go up behind one copy command per batch,
        other scans behind one per frame.  Device tensors are refused (ValueError): copying them with hipMemcpyDefault would change
        the copy of the measured one-block path, and ``run`` takes them as they are.  ``exact_patches``, ``calib_angle``: as in ``run`` (the
        correction runs on the device slot's copy, after it has landed)."""
        k, B = len(host_scans), self.batch
        out = out or FrameBatch(self.eng, k)
        assert out.k >= k and (not pairs or len(rands) >= k) and ahead >= 1
        for pc in host_scans:
            assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] == 4 and pc.is_contiguous()
            if pc.is_cuda:
                raise ValueError("Pipeline.run_uploading takes scans in host memory; Pipeline.run takes device scans")
        src = np.array([pc.data_ptr() for pc in host_scans], dtype=np.uint64)
        nbytes = np.array([int(pc.shape[0]) * 16 for pc in host_scans], dtype=np.uint64)
        # A producer that leaves the scans of a batch in ONE pinned block at a fixed pitch (run_sequence.py's loader does) gets one
        # copy command per batch: the device slots mirror the pitch.  Measured (tools/upload_contention_probe.py): eight 2 MB copies per
        # batch cost a resident pipeline running beside them 20 % (41 GB/s), one 16 MB copy 0-3 % (54 GB/s) -- the commands, not the
        # bytes, are what the copies cost.
        pitch = 0
        if k > 1:
            d = np.diff(src.astype(np.int64))
            inside = np.ones(k - 1, bool); inside[B - 1::B] = False          # (the step from one batch to the next may be anything)
            if inside.any() and (d[inside] == d[inside][0]).all() and int(d[inside][0]) >= int(nbytes.max()) and int(d[inside][0]) % 16 == 0:
                # ... and the scans of a batch must be views of ONE allocation that spans the whole copy: equal spacing alone would also
                # be true of separately pinned tensors that happen to sit at a fixed distance, and one copy over them would read the gaps
                stor = [(pc.untyped_storage().data_ptr(), pc.untyped_storage().nbytes()) for pc in host_scans]
                one_block = all(len({stor[i][0] for i in range(lo, min(k, lo + B))}) == 1 and
                                int(src[min(k, lo + B) - 1] + nbytes[min(k, lo + B) - 1]) <= stor[lo][0] + stor[lo][1]
                                for lo in range(0, k, B))
                if one_block:
                    pitch = int(d[inside][0])
        # a slot holds a batch, frame i at (i % B) * stride: the pitch, or the engine's scan capacity (a later call with a slightly
        # longer scan must not find itself allocating device memory behind the caller's clock)
        stride = pitch or 16 * max(int(nbytes.max()) // 16, int(self.eng.max_points))
        first = np.arange(0, k, B)
        last = np.minimum(first + B, k) - 1

        def build(fb):
            pcs = fb + (np.arange(k, dtype=np.uint64) % np.uint64(B)) * np.uint64(stride)
            jobs = self._jobs(pcs, nbytes // np.uint64(16), rands, prev, out, pairs, dist_channels, False, dedup, certify, rands_host, exact_patches,
                              calib_angle)
            if pitch:   # one copy per batch: first frame's slot, first frame's source, bytes up to the end of the last frame
                return jobs, (pcs[first], src[first], src[last] + nbytes[last] - src[first], np.arange(len(first) + 1))
            return jobs, (pcs, src, nbytes, np.r_[first, k])   # one copy per frame
        return self._upload_run(k, ahead, B * stride, build, out, certify, pairs)

    def run_loaded(self, loader, b0, nb, prev=None, out=None, pairs=True, dist_channels=5, dedup=True, certify=True, ahead=4, publish=True,
                   exact_patches=False, calib_angle=None):
        """Batches [b0, b0 + nb) of a SeqLoader through the pipeline: a batch's scans AND draws go up behind ONE copy command (the loader's
        slot layout, mirrored on the device), the jobs are built column-wise for the whole call, and nothing here is per-frame Python.
        The loop of ``run_uploading``, fed by the loader.  A device slot here also holds the batch's draws, which its PAIR stage reads:
        before the copy that overwrites the slot of batch b - 2 the calling thread waits for an event recorded on the pair stream after
        that batch's pairs (the encoder wait of ``run_uploading`` does not cover them).  With ``certify`` the certifier reads the draws
        from the loader's keep ring, which must hold ring + 7 batches (caelo_pipeline::CERT_RING + 1 beyond the loader's ring; refused
        otherwise).  ``exact_patches``, ``calib_angle``: as in ``Pipeline.run``.  -> (FrameBatch, frames)."""
        B = self.batch
        assert loader.batch == B and ahead >= 1 and b0 + nb <= loader.n_batches
        k = min(loader.n - b0 * B, nb * B)
        out = out or FrameBatch(self.eng, k)
        assert out.k >= k
        f = np.arange(k, dtype=np.uint64)
        lb, j = f // B, f % B                                # local batch, frame within it
        rnd_h = np.uint64(loader.keep_h.ctypes.data) + (((b0 + lb) % np.uint64(loader.keep_n)) * np.uint64(B) + j) * np.uint64(6000 * 8)

        def build(fb):   # a slot: the batch's scans at the loader's capacity, then its draws
            return self._jobs(fb + j * np.uint64(loader.cap * 16), np.zeros(k, np.int64), fb + np.uint64(loader.scan_bytes) + j * np.uint64(6000 * 8),
                              prev, out, pairs, dist_channels, False, dedup, certify, rnd_h if certify else None, exact_patches, calib_angle), None
        return self._upload_run(k, ahead, loader.slot_bytes, build, out, certify, pairs, publish, loader, b0), k

    def _upload_run(self, k, ahead, slot_bytes, build, out, certify, pairs, publish=True, loader=None, b0=0):
        """The end of both upload modes: ``ahead + 2`` device slots of ``slot_bytes`` each (one set per Pipeline, replaced when a call
        needs another layout), one copy stream, ONE call of caelo_pipeline_run_uploading, the exact results.  ``build(fb)``, with
        fb [k] the device address of frame i's slot (batch b0 + i // batch goes to slot (b0 + i // batch) % slots) -> (jobs, copy table
        (dst, src, bytes, copy_first) or None with a loader).  Host times of the call in ``last_upload_times`` (ms)."""
        eng, B, slots = self.eng, self.batch, ahead + 2
        if self._slots is None or self._slots[0] != (slots, slot_bytes):
            self._slots = ((slots, slot_bytes), [torch.empty((slot_bytes,), dtype=torch.uint8, device=eng.device) for _ in range(slots)])
        if self._copy is None:
            self._copy = torch.cuda.Stream(device=eng.device)
        base = np.array([t.data_ptr() for t in self._slots[1]], dtype=np.uint64)
        t0 = time.perf_counter()
        jobs, table = build(base[(b0 + np.arange(k) // B) % slots])
        if table is None:
            dst, src, nbytes, first = base, None, None, None
        else:   # (kept alive by these names until the call returns)
            dst, src, nbytes = (np.ascontiguousarray(a, dtype=np.uint64) for a in table[:3])
            first = np.ascontiguousarray(table[3], dtype=np.int64)

        def addr(a):
            return None if a is None else C.c_void_p(a.ctypes.data)
        tns = (C.c_int64 * 4)()
        t1 = time.perf_counter()
        _ffi.check(eng.lib.caelo_pipeline_run_uploading(self.h, addr(jobs), k, (k + B - 1) // B, loader.h if loader else None, int(b0), addr(dst),
                                                        addr(src), addr(nbytes), addr(first), slots,
                                                        C.c_void_p(loader.ring_h.data_ptr()) if loader else None, loader.slot_bytes if loader else 0,
                                                        int(ahead), C.c_void_p(self._copy.cuda_stream), eng.stream, tns))
        t2 = time.perf_counter()
        self._finish_exact(out, k, certify, pairs, publish)
        self.last_upload_times = dict(starved_ms=tns[0] / 1e6, wait_arrival_ms=tns[1] / 1e6, submit_ms=tns[2] / 1e6, upload_and_pace_ms=tns[3] / 1e6,
                                      jobs_ms=1e3 * (t1 - t0), native_loop_ms=1e3 * (t2 - t1), publish_ms=1e3 * (time.perf_counter() - t2))
        return out


class SeqLoader:
    """caelo_seqloader (include/caelo.h, csrc/seqload.hip): native threads read the scan files of a sequence batch after batch into a
    pinned ring and generate each pair's RANSAC draws (NumPy's MT19937 stream, bit for bit).  ``Pipeline.run_loaded`` consumes it."""

    def __init__(self, eng, paths, first_frame=0, batch=8, seed_base=1000, threads=16, ring=10, keep=96, cap=None):
        import os
        self.eng, lib = eng, eng.lib
        self.batch, self.cap, self.n = int(batch), int(cap or eng.max_points), len(paths)
        self.ring, self.keep_n = int(ring), int(keep)
        self.n_batches = (self.n + self.batch - 1) // self.batch
        self.slot_bytes = int(lib.caelo_seqloader_slot_bytes(self.batch, self.cap))
        self.scan_bytes = self.batch * self.cap * 16
        self.ring_h = torch.empty((self.ring, self.slot_bytes), dtype=torch.uint8, pin_memory=True)
        self.keep_h = np.empty((self.keep_n, self.batch, 6000), np.float64)
        self._arr = (C.c_char_p * self.n)(*[os.fsencode(p_) for p_ in paths])
        h = C.c_void_p()
        _ffi.check(lib.caelo_seqloader_create(self._arr, self.n, int(first_frame), self.batch, self.ring, self.cap, C.c_void_p(self.ring_h.data_ptr()),
                                              C.c_void_p(self.keep_h.ctypes.data), self.keep_n, int(seed_base), int(threads), C.byref(h)))
        self.h = h
        self._slot = C.c_int32(0)
        self._npts = (C.c_int64 * self.batch)()

    def wait(self, b):
        """-> (ring slot, point counts of the batch's frames [batch] int64); blocks until batch b is loaded."""
        _ffi.check(self.eng.lib.caelo_seqloader_wait(self.h, int(b), C.byref(self._slot), self._npts))
        return int(self._slot.value), np.frombuffer(self._npts, dtype=np.int64).copy()

    def release(self, b):
        _ffi.check(self.eng.lib.caelo_seqloader_release(self.h, int(b)))

    def stats(self):
        o = (C.c_int64 * 3)()
        _ffi.check(self.eng.lib.caelo_seqloader_stats(self.h, o))
        return {"read_s": o[0] / 1e9, "draws_s": o[1] / 1e9, "wait_slot_s": o[2] / 1e9}

    def close(self):
        if self.h:
            self.eng.lib.caelo_seqloader_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, respond_h5=RESPOND_H5, encoder_h5=ENCODER_H5, device=None, max_points=160000):
        if not torch.cuda.is_available():
            raise _ffi.CaeloError("no HIP device visible: libcaelo has no CPU fallback")
        self.lib = _ffi.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        _ffi.check(self.lib.caelo_create(C.byref(ctx), self.device_index))
        self.ctx = ctx
        self.max_points = int(max_points)
        self._maps = {}
        self._wss = {}      # (HIP stream, kind) -> scratch bytes: workspaces and voxel maps are per stream, so
                            # frames issued on different streams ("lanes") run concurrently without sharing scratch
        if respond_h5:
            self.load_weights(respond_h5)
        if encoder_h5:
            self.load_weights(encoder_h5)

    def __del__(self):
        try:
            self._maps.clear()
            if self.ctx:
                self.lib.caelo_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ---- plumbing ----------------------------------------------------------------------------
    @property
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def load_weights(self, path):
        """A Keras .h5 of either network.  An encoder file always sets ITS activations with its weights: loading the shipped file
        after a relu model restores tanh / tanh."""
        kind, ws, activations = read_keras_model(path)
        if kind == "respond":
            self.set_respond_weights(ws)
        else:
            self.set_encoder_weights(ws, activations=activations)
        return kind

    @staticmethod
    def _weight_arrays(ws, shapes, what):
        """A caller's weight list as contiguous f32 arrays; ValueError unless array i has the Keras shape ``shapes[i]`` (kernel then
        bias per layer) or is that many elements flat."""
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w in ws]
        ok = len(ws) == len(shapes) and all(w.shape == s or w.shape == (int(np.prod(s)),) for w, s in zip(ws, shapes))
        if not ok:
            raise ValueError("%s weights: %d arrays of shapes %s wanted, got %s" % (what, len(shapes), list(shapes), [w.shape for w in ws]))
        return ws

    def set_encoder_weights(self, ws, activations=None):
        """caelo_set_encoder_weights / caelo_set_encoder_model: the ten arrays of the encoder (conv3d_1..3, dense_1, dense_2: kernel,
        bias each) as float32 arrays in Keras layout.  ``activations``: (hidden, code), hidden in ("tanh", "relu") for the four hidden
        layers, code in ("tanh", "linear") for dense_2; None keeps the engine's current pair (tanh / tanh until one is set).  Every
        derived operand image of the context is rebuilt; work already issued is waited for first.  A relu model whose activations can
        leave the f16 range of the split operands (encoder_range) is refused with a CaeloError naming the layer; the engine then
        still holds its previous model."""
        ws = self._weight_arrays(ws, ENCODER_SHAPES, "encoder")
        codes = None if activations is None else _activation_codes(activations)
        torch.cuda.synchronize(self.device)
        if codes is None:
            _ffi.check(self.lib.caelo_set_encoder_weights(self.ctx, *[_hptr(w) for w in ws]))
        else:
            _ffi.check(self.lib.caelo_set_encoder_model(self.ctx, *([_hptr(w) for w in ws] + [codes[0], codes[1]])))

    def encoder_activations(self):
        """caelo_get_encoder_activations -> (hidden, code) of the engine's encoder, e.g. ("tanh", "tanh")."""
        out = (C.c_int32 * 2)()
        _ffi.check(self.lib.caelo_get_encoder_activations(self.ctx, C.cast(out, C.c_void_p)))
        return ACTIVATION_NAMES[int(out[0])], ACTIVATION_NAMES[int(out[1])]

    @staticmethod
    def encoder_range(ws, activations):
        """caelo_host_encoder_range (host only, no device): -> (bounds [5] f64, over) -- the worst-case magnitude of each layer's
        output over binary patches (1 behind a tanh layer), and the name of the first layer whose output a kernel splits into f16
        halves and that can exceed 65504 (conv3d_1..3), or None when the model is in range."""
        ws = Engine._weight_arrays(ws, ENCODER_SHAPES, "encoder")
        h, c = _activation_codes(activations)
        out = (C.c_double * 5)()
        rc = _ffi.load().caelo_host_encoder_range(*([_hptr(w) for w in ws] + [h, c, C.cast(out, C.c_void_p)]))
        if rc < 0:
            _ffi.check(rc)
        return np.array(out, np.float64), (ENCODER_LAYERS[rc - 1] if rc > 0 else None)

    def set_decoder_weights(self, ws, activations):
        """caelo_set_decoder_model: the ten arrays of the decoder (dense_3, dense_4, conv3d_4, conv3d_5, conv3d_6: kernel, bias each) as
        float32 arrays in Keras layout and ``activations`` = (hidden, out), hidden in ("tanh", "relu") for the four hidden layers, out
        "sigmoid".  Work already issued is waited for first.  The encoder and everything else of the engine are untouched."""
        ws = self._weight_arrays(ws, DECODER_SHAPES, "decoder")
        try:
            h, o = activations
            h = ACTIVATION_CODES[h] if isinstance(h, str) else int(h)
            o = _ffi.ACT_SIGMOID if o == "sigmoid" else int(o)
        except (KeyError, TypeError, ValueError):
            h = o = -1
        if h not in (_ffi.ACT_TANH, _ffi.ACT_RELU) or o != _ffi.ACT_SIGMOID:
            raise ValueError("decoder activations: (hidden, out) with hidden in ('tanh', 'relu') and out 'sigmoid', got %r" % (activations,))
        torch.cuda.synchronize(self.device)
        _ffi.check(self.lib.caelo_set_decoder_model(self.ctx, *([_hptr(w) for w in ws] + [h, o])))

    def decoder_activations(self):
        """caelo_get_decoder_activations -> (hidden, out) of the engine's decoder, e.g. ("relu", "sigmoid"); CaeloError when none is set."""
        out = (C.c_int32 * 2)()
        _ffi.check(self.lib.caelo_get_decoder_activations(self.ctx, C.cast(out, C.c_void_p)))
        return ACTIVATION_NAMES[int(out[0])], ACTIVATION_NAMES[int(out[1])]

    def load_autoencoder(self, path, encoder_h5=None):
        """A Keras autoencoder .h5 (AE4VoxelPatch.py's AutoencoderModel4VoxelPatch.h5): sets the encoder, exactly as ``load_weights``
        does for that file, and the decoder.  ``encoder_h5``: where the encoder's weights are when ``path`` was cut down to the
        decoder's (the test fixtures are stored that way); by default ``path`` must hold both halves.
        -> ((H, C), (hidden, out)).  Both layer stacks are checked before a weight is read or the engine is changed."""
        from . import keras_config
        enc, enc_acts, dec, dec_acts = keras_config.read_autoencoder(path)
        if dec is None:
            raise ValueError("%s holds no decoder weights" % path)
        if encoder_h5 is not None:
            kind, enc, enc_acts = read_keras_model(encoder_h5)
            if kind != "encoder":
                raise ValueError("%s is not a voxel-patch encoder" % encoder_h5)
        elif enc is None:
            raise ValueError("%s holds no encoder weights (pass encoder_h5=)" % path)
        self.set_encoder_weights(enc, activations=enc_acts)
        self.set_decoder_weights(dec, dec_acts)
        return enc_acts, dec_acts

    def set_respond_weights(self, ws):
        """caelo_set_respond_weights: conv2d_1 and conv2d_2 of the response layer (kernel, bias each), float32 arrays in Keras layout."""
        ws = self._weight_arrays(ws, RESPOND_SHAPES, "response-layer")
        torch.cuda.synchronize(self.device)
        _ffi.check(self.lib.caelo_set_respond_weights(self.ctx, *[_hptr(w) for w in ws]))

    def _ws(self, kind, need):
        """Scratch bytes of the current stream for one entry point (grown on demand, never shared across streams)."""
        key = (torch.cuda.current_stream(self.device).cuda_stream, kind)
        t = self._wss.get(key)
        if t is None or t.numel() < need:
            # zero-filled: caelo_match / caelo_ransac keep their tickets in the workspace and leave them zero
            t = self._wss[key] = torch.zeros(int(need), dtype=torch.uint8, device=self.device)
        return t

    def set_encoder_reference(self, on=True):
        """caelo_set_encoder_reference: stage 1 of this engine's encoder = the exact-f32 kernel (precision reference; slower)."""
        _ffi.check(self.lib.caelo_set_encoder_reference(self.ctx, 1 if on else 0))

    def set_calib_angle(self, deg):
        """caelo_set_calib_angle: the angle (degrees) the CAELO_EXTRACT_CORRECT_PC mode rotates scans by; a context setting like the
        weights (0 until set).  ValueError for a non-finite angle."""
        deg = float(deg)
        if not np.isfinite(deg):
            raise ValueError("the calibration angle must be a finite number of degrees (got %r)" % (deg,))
        _ffi.check(self.lib.caelo_set_calib_angle(self.ctx, deg))

    def get_calib_angle(self):
        return float(self.lib.caelo_get_calib_angle(self.ctx))

    def _calib_frames(self, calib_angle, k):
        """``calib_angle=`` of the pipeline's job builder: a number (every frame) or one entry per frame (the angle, or None for a frame
        that is not corrected; the context holds ONE angle, so the entries that are not None must agree).  Sets the context's angle ->
        bool [k], the frames that get the mode bit."""
        if np.isscalar(calib_angle):
            on, angles = np.ones(k, dtype=bool), {float(calib_angle)}
        else:
            assert len(calib_angle) == k, "calib_angle: a number, or one entry per frame"
            on = np.array([a is not None for a in calib_angle], dtype=bool)
            angles = {float(a) for a in calib_angle if a is not None}
        if len(angles) > 1:
            raise ValueError("one calibration angle per run (got %s): the angle is a context setting" % sorted(angles))
        if angles:
            self.set_calib_angle(angles.pop())
        return on

    def correct_pc(self, pc, angle):
        """caelo_correct_pc (CorrectPC, Transformations.py:28-39): pc [N,3] or [N,4] f32 (device) rotated point by point by ``angle``
        degrees about p x z^ -> a new tensor of the same shape; column 3 (intensity) is copied bit for bit.  No host sync.  A point with
        x = y = 0 becomes NaN, as in the Python reference."""
        assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] in (3, 4) and pc.is_contiguous()
        angle = float(angle)
        if not np.isfinite(angle):
            raise ValueError("the calibration angle must be a finite number of degrees (got %r)" % (angle,))
        out = torch.empty_like(pc)
        _ffi.check(self.lib.caelo_correct_pc(self.ctx, _ptr(pc), pc.shape[0], pc.shape[1], angle, _ptr(out), self.stream))
        return out

    def lane_faults(self):
        """caelo_lane_faults: wavefronts of the pose kernels whose lanes disagreed on a hypothesis they all derive from the
        same inputs, plus descriptors the encoder wrote that are not finite or, under a tanh code, not within [-1, 1] (self-checks of the two
        halves; synchronises).  0 on healthy hardware with sane weights."""
        out = C.c_int64(0)
        _ffi.check(self.lib.caelo_lane_faults(self.ctx, C.byref(out)))
        return int(out.value)

    def pipeline(self, batch=4, buffers=3):
        """The native frame executor (caelo_pipeline): `batch` frames per launch, `buffers` batches of patches in flight
        between the front and the encoder; created once per configuration."""
        key = ("pipeline", int(batch), int(buffers))
        if key not in self._maps:
            self._maps[key] = Pipeline(self, batch, buffers)
        return self._maps[key]

    def voxmap(self, max_points=None, slot=0):
        n = self.max_points if max_points is None else int(max_points)
        key = (torch.cuda.current_stream(self.device).cuda_stream, slot, n)
        if key not in self._maps:
            self._maps[key] = VoxelMap(self, n)
        return self._maps[key]

    def _encode_ws(self, n_patches):
        return self._ws("encode", int(self.lib.caelo_encode_ws_bytes(int(n_patches))))

    # ---- stages (device tensors in, device tensors out, no sync) ---------------------------------
    def project(self, pc, status=None):
        assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] == 4 and pc.is_contiguous()
        ring = self.empty((RING_H, RING_W, RING_C), torch.float32)
        counter = self.empty((RING_H, RING_W), torch.int32)
        winner = self.empty((RING_H * RING_W,), torch.int32)
        status = self.zeros((1,), torch.int32) if status is None else status
        _ffi.check(self.lib.caelo_project(self.ctx, _ptr(pc), pc.shape[0], _ptr(ring), _ptr(counter), _ptr(winner),
                                          _ptr(status), self.stream))
        return ring, counter, status

    def respond(self, img):
        """img [rows>=64, w>=1792, c>=3] f32 -> [64,1792,8]."""
        assert img.dtype == torch.float32 and img.dim() == 3 and img.is_contiguous()
        resp = self.empty((NET_H, NET_W, 8), torch.float32)
        _ffi.check(self.lib.caelo_respond(self.ctx, _ptr(img), img.shape[1], img.shape[2], _ptr(resp), self.stream))
        return resp

    def keypoints(self, ring, counter, resp, status=None):
        assert ring.dtype == torch.float32 and counter.dtype == torch.int32 and resp.dtype == torch.float32
        assert ring.is_contiguous() and counter.is_contiguous() and resp.is_contiguous()
        kpix = self.zeros((MAX_K, 2), torch.int64)
        kpts = self.zeros((MAX_K, 3), torch.float32)
        nkey = self.empty((1,), torch.int32)
        status = self.zeros((1,), torch.int32) if status is None else status
        _ffi.check(self.lib.caelo_keypoints(self.ctx, _ptr(ring), ring.shape[1], ring.shape[2], _ptr(counter),
                                            counter.shape[1], _ptr(resp), _ptr(self._ws("keypoints", self.lib.caelo_keypoints_ws_bytes())),
                                            _ptr(kpix), _ptr(kpts),
                                            _ptr(nkey), _ptr(status), self.stream))
        return kpts, kpix, nkey, status

    def planar_points(self, ring, counter, resp):
        """Planar points with normals (caelo_planar_points; SphericalRing.py:236-282) from what ``keypoints`` takes.
        -> (planar [PLANAR_MAX,6] f32 = xyz | normal with n_z > 0, pixels [PLANAR_MAX,2] i32 (row, col), n [1] i32): rows 0 .. n - 1
        in row-major pixel order, zeros behind them.  No synchronisation."""
        assert ring.dtype == torch.float32 and counter.dtype == torch.int32 and resp.dtype == torch.float32
        assert ring.is_contiguous() and counter.is_contiguous() and resp.is_contiguous()
        planar = self.zeros((_ffi.PLANAR_MAX, 6), torch.float32)
        pixels = self.zeros((_ffi.PLANAR_MAX, 2), torch.int32)
        n = self.empty((1,), torch.int32)
        _ffi.check(self.lib.caelo_planar_points(self.ctx, _ptr(ring), ring.shape[1], ring.shape[2], _ptr(counter), counter.shape[1],
                                                _ptr(resp), _ptr(self._ws("planar", self.lib.caelo_planar_ws_bytes())), _ptr(planar),
                                                _ptr(pixels), _ptr(n), self.stream))
        return planar, pixels, n

    def scan_context(self, pts, n_pts):
        """Scan Context descriptors (caelo_scan_context): pts [F,Nmax,C] f32 (C 3 or 4), n_pts [F] i32 ->
        (sc [F,20,60] f32, u [F,1200] f32 unit columns, valid [F] i64: bit c = column c is not empty).  No synchronisation."""
        assert pts.dtype == torch.float32 and pts.dim() == 3 and pts.is_contiguous() and n_pts.dtype == torch.int32 and n_pts.is_contiguous()
        f = pts.shape[0]
        assert n_pts.shape == (f,)
        sc = self.zeros((f, _ffi.SC_RINGS, _ffi.SC_SECTORS), torch.float32)
        u = self.zeros((f, _ffi.SC_RINGS * _ffi.SC_SECTORS), torch.float32)
        valid = self.zeros((f,), torch.int64)
        ws = self._ws("scan_context", int(self.lib.caelo_sc_ws_bytes(f)))
        _ffi.check(self.lib.caelo_scan_context(self.ctx, _ptr(pts), pts.shape[1], pts.shape[2], _ptr(n_pts), f, _ptr(sc), _ptr(u),
                                               _ptr(valid), _ptr(ws), self.stream))
        return sc, u, valid

    def loop_search(self, u, valid, min_gap=50, k=1, max_dist=None, min_cols=1, queries=None, dense=False):
        """The all-pairs column-shifted search (caelo_loop_search) over what ``scan_context`` returns: for every query
        i of ``queries`` = (q0, q1) (all frames when None) the k best candidates j <= i - min_gap by (distance, lower j), only those
        below max_dist when given.  -> (cand [Nq,k] i32, dist [Nq,k] f32, shift [Nq,k] i32), empty slots -1 / +inf / -1; dense = True
        adds (dist [Nq,N] f32, shift [Nq,N] i8) over every pair, +inf / -1 outside the candidates.  Turning scan i by shift * 6 degrees
        about z brings it to j's heading.  No synchronisation."""
        assert u.dtype == torch.float32 and u.dim() == 2 and u.is_contiguous() and valid.dtype == torch.int64 and valid.is_contiguous()
        n = u.shape[0]
        q0, q1 = (0, n) if queries is None else (int(queries[0]), int(queries[1]))
        nq = max(q1 - q0, 0)
        cand = self.empty((nq, k), torch.int32)
        dist = self.empty((nq, k), torch.float32)
        shift = self.empty((nq, k), torch.int32)
        dd = self.empty((nq, n), torch.float32) if dense else None
        ds = self.empty((nq, n), torch.int8) if dense else None
        if nq == 0:   # (an empty tensor has no address to hand over)
            return (cand, dist, shift, dd, ds) if dense else (cand, dist, shift)
        ws = self._ws("loop_search", max(16,int(self.lib.caelo_loop_search_ws_bytes(n, q0, q1, int(min_gap), int(k)))))
        _ffi.check(self.lib.caelo_loop_search(self.ctx, _ptr(u), _ptr(valid), n, q0, q1, int(min_gap), int(k),
                                              float("inf") if max_dist is None else float(max_dist), int(min_cols), _ptr(cand), _ptr(dist),
                                              _ptr(shift), _ptr(dd), _ptr(ds), _ptr(ws), self.stream))
        return (cand, dist, shift, dd, ds) if dense else (cand, dist, shift)

    def extend_keypts(self, ring, counter, key_pixels, n_key=None):
        """ExtendKeyPtsInShpericalRing on device tensors: ring [H,W,C] f32, counter [Hc,Wc] i32 (MUTATED: the windows
        are zeroed like SphericalRing.py:307), key_pixels [K,2] i64 -> (ext_pts [K*169,3] f32, n_ext [1] i32)."""
        assert ring.dtype == torch.float32 and counter.dtype == torch.int32 and key_pixels.dtype == torch.int64
        assert ring.is_contiguous() and counter.is_contiguous() and key_pixels.is_contiguous()
        rows, cols = min(ring.shape[0], counter.shape[0]), min(ring.shape[1], counter.shape[1])
        k = key_pixels.shape[0]
        ext = self.empty((k * 169, 3), torch.float32)
        n_ext = self.empty((1,), torch.int32)
        ws = self._ws("extend", int(self.lib.caelo_extend_ws_bytes(rows, cols)))
        _ffi.check(self.lib.caelo_extend_keypts(self.ctx, _ptr(ring), ring.shape[1], ring.shape[2], _ptr(counter), counter.shape[1],
                                                rows, cols, _ptr(key_pixels), k, _ptr(n_key), _ptr(ext), _ptr(n_ext), _ptr(ws),
                                                self.stream))
        return ext, n_ext

    def icp_step(self, pc0, pc1, threshold, min_inliers=100):
        """One ICP iteration (caelo_icp_step): pc1 [n1,3] f32 is moved IN PLACE.  -> (rt [12] f32, n_inliers [1] i32)."""
        for t in (pc0, pc1):
            assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous()
        rt = self.empty((12,), torch.float32)
        n_in = self.empty((1,), torch.int32)
        ws = self._ws("icp", int(self.lib.caelo_icp_ws_bytes(pc1.shape[0])))
        _ffi.check(self.lib.caelo_icp_step(self.ctx, _ptr(pc0), pc0.shape[0], _ptr(pc1), pc1.shape[0], float(threshold),
                                           int(min_inliers), _ptr(rt), _ptr(n_in), _ptr(ws), self.stream))
        return rt, n_in

    def icp(self, pc0, pc1, planar0=None, planar1=None, nn="brute", **kw):
        """The reference's ICP loops entirely on the device (caelo_icp): pc1 [n1,3] (and planar1 [m1,6]) are MOVED in place.
        kw: threshold0/1, decay0/1, small_shift, ep, max_iter, min_iter, min_pairs, fail_only_first.  -> IcpResult bytes tensor
        (read it with ``icp_result``: the only synchronisation).  nn = "grid": the nearest neighbours come from a cell grid over
        frame 0 (caelo_icp_grid: the same pairs and bits; it refuses growing thresholds and non-finite coordinates, and
        synchronises once on entry)."""
        if nn not in ("brute", "grid"):
            raise ValueError("nn must be 'brute' or 'grid', not %r" % (nn,))
        for t in (pc0, pc1):
            assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous()
        use_planar = planar0 is not None
        if use_planar:
            for t in (planar0, planar1):
                assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and (t.shape[0] == 0 or t.shape[1] == 6)
        prm = _ffi.IcpParams(threshold0=kw.get("threshold0", 0.5), threshold1=kw.get("threshold1", 2.0), decay0=kw.get("decay0", 0.9),
                             decay1=kw.get("decay1", 0.5), small_shift=kw.get("small_shift", 0.05), ep=kw.get("ep", 0.001),
                             max_iter=kw.get("max_iter", 50), min_iter=kw.get("min_iter", 19), min_pairs=kw.get("min_pairs", 100),
                             fail_only_first=kw.get("fail_only_first", 0), use_planar=1 if use_planar else 0, reserved=0)
        m0 = planar0.shape[0] if use_planar else 0
        m1 = planar1.shape[0] if use_planar else 0
        res = self.empty((C.sizeof(_ffi.IcpResult),), torch.uint8)
        if nn == "grid":
            lay = (C.c_int64 * 8)()
            _ffi.check(self.lib.caelo_icp_grid_ws_layout(pc0.shape[0], pc1.shape[0], m0, m1, C.cast(lay, C.c_void_p)))
            ws, fn = self._ws("icp_grid", int(lay[7])), self.lib.caelo_icp_grid
        else:
            ws, fn = self._ws("icp_loop", int(self.lib.caelo_icp_loop_ws_bytes(pc1.shape[0], m1))), self.lib.caelo_icp
        _ffi.check(fn(self.ctx, _ptr(pc0), pc0.shape[0], _ptr(pc1), pc1.shape[0], _ptr(planar0) if m0 else None, m0,
                      _ptr(planar1) if m1 else None, m1, C.byref(prm), _ptr(res), _ptr(ws), self.stream))
        return res

    @staticmethod
    def icp_result(res):
        """Synchronising read of a caelo_icp_result."""
        return _ffi.IcpResult.from_buffer_copy(res.cpu().numpy().tobytes())

    def kp_nn_pairs(self, pts, n_key, pairs, thresholds, want_dist=True):
        """Key point repeatability on the device (caelo_kp_nn_pairs, EvaluationOnKeypts.py:68-94, :128-140).

        pts [F, ld, 3] f64 world-frame key points (frame f: rows 0 .. n_key[f]-1), n_key [F] int, pairs [P, 2] int = (fit frame,
        query frame), thresholds: 1 to 16 finite positive floats.  -> (dist [P, ld] f64 with NaN past each query frame's n_key, or
        None; counts [P, T + 1] i64), on the device.  dist is scikit-learn's kd-tree distance to the nearest fit point, bit for bit.

        Refused with ValueError before any launch (include/caelo.h): a fit set of 3 points or fewer (scikit-learn answers those by
        brute force, with a dot-product formula and BLAS rounding), a query set of none, a non-finite coordinate (scikit-learn raises
        there too), ld above CAELO_KP_NN_MAX_K, a pair index out of range, thresholds that are not finite and positive."""
        pts = torch.as_tensor(pts, dtype=torch.float64, device=self.device).contiguous()
        if pts.dim() != 3 or pts.shape[2] != 3:
            raise ValueError("pts must be [F, ld, 3], got %s" % (tuple(pts.shape),))
        F, ld = int(pts.shape[0]), int(pts.shape[1])
        if ld < 1 or ld > _ffi.KP_NN_MAX_K:
            raise ValueError("ld = %d: a key point set holds 1 to %d points here" % (ld, _ffi.KP_NN_MAX_K))
        nk = np.asarray(n_key.cpu() if torch.is_tensor(n_key) else n_key, dtype=np.int64).reshape(-1)
        pr = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, dtype=np.int64).reshape(-1, 2)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        if nk.shape[0] != F:
            raise ValueError("n_key holds %d counts for %d frames" % (nk.shape[0], F))
        if not 1 <= thr.size <= _ffi.KP_NN_MAX_THRESHOLDS or not (np.isfinite(thr).all() and (thr > 0).all()):
            raise ValueError("thresholds: 1 to %d finite positive values, got %s" % (_ffi.KP_NN_MAX_THRESHOLDS, thr.tolist()))
        if pr.size and (pr.min() < 0 or pr.max() >= F):
            raise ValueError("a pair names a frame outside [0, %d)" % F)
        if ((nk < 0) | (nk > ld)).any():
            raise ValueError("n_key must lie in [0, ld = %d]" % ld)
        if pr.size:
            small = [int(f) for f in np.unique(pr[:, 0]) if nk[f] <= 3]
            if small:
                raise ValueError("fit set(s) of frame(s) %s hold 3 points or fewer: scikit-learn brute-forces those (a different "
                                 "rounding), which this kernel does not restate" % small[:10])
            empty = [int(f) for f in np.unique(pr[:, 1]) if nk[f] < 1]
            if empty:
                raise ValueError("query set(s) of frame(s) %s are empty" % empty[:10])
        nk_d = torch.from_numpy(nk.astype(np.int32)).to(self.device)
        inside = torch.arange(ld, device=self.device)[None, :] < nk_d[:, None]
        if not bool(torch.isfinite(pts[inside]).all()):
            raise ValueError("Input contains NaN, infinity or a value too large for dtype('float64').")
        pr_d = torch.from_numpy(pr.astype(np.int32)).to(self.device).contiguous()
        P = pr.shape[0]
        dist = torch.full((P, ld), float("nan"), dtype=torch.float64, device=self.device) if want_dist else None
        counts = self.empty((P, thr.size + 1), torch.int64)
        _ffi.check(self.lib.caelo_kp_nn_pairs(self.ctx, _ptr(pts), F, ld, _ptr(nk_d), _ptr(pr_d), P, _hptr(thr), int(thr.size),
                                              _ptr(dist), _ptr(counts), self.stream))
        return dist, counts

    def _detector_frames(self, pts, n_pts, name):
        """The input checks iss_keypoints and harris_keypoints share -> (pts [F, ld, 3] f32 contiguous, n_pts [F] i32 on the device,
        whether pts came as one cloud [n, 3]).  ValueError for a wrong shape or dtype, ld above CAELO_ISS_MAX_POINTS, n_pts of the wrong
        length or outside [0, ld], and -- the one read-back -- a non-finite coordinate in a frame's rows."""
        from . import iss
        pts = torch.as_tensor(pts, device=self.device)
        single = pts.dim() == 2
        if single:
            pts = pts[None]
        if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32:
            raise ValueError("pts must be float32 [F, ld, 3] or [n, 3], got %s %s" % (pts.dtype, tuple(pts.shape[1:] if single else pts.shape)))
        pts = pts.contiguous()
        F, ld = int(pts.shape[0]), int(pts.shape[1])
        if ld > iss.MAX_POINTS:
            raise ValueError("ld = %d: %s takes at most %d points per frame (an all-pairs search; subsample the scan)" % (ld, name, iss.MAX_POINTS))
        if n_pts is None:
            np_d = torch.full((F,), ld, dtype=torch.int32, device=self.device)
        else:
            np_d = torch.as_tensor(n_pts, device=self.device).reshape(-1)
            if np_d.shape[0] != F or np_d.dtype.is_floating_point:
                raise ValueError("n_pts holds %d counts (%s) for %d frames" % (np_d.shape[0], np_d.dtype, F))
            if F and ld and bool(((np_d < 0) | (np_d > ld)).any()):
                raise ValueError("n_pts must lie in [0, ld = %d]" % ld)
            np_d = np_d.to(torch.int32).contiguous()
        if F and ld:
            inside = torch.arange(ld, device=self.device)[None, :] < np_d[:, None]
            if not bool(torch.isfinite(pts[inside]).all()):
                raise ValueError("%s: a point has a non-finite coordinate" % name)
        return pts, np_d, single

    def _detect(self, sym, name, pts, n_pts, cp, outputs, entry="keypoints"):
        """What iss_keypoints, harris_keypoints and sift_octave share round caelo_<sym>_<entry>: the frames checked (_detector_frames),
        key_idx and n_key allocated beside the detector's three ``outputs(F, ld)`` (in the C order; None = not wanted), the workspace
        fetched, the call -> [key_idx, n_key, *outputs], without the frame axis for a single cloud."""
        pts, np_d, single = self._detector_frames(pts, n_pts, name)
        F, ld = int(pts.shape[0]), int(pts.shape[1])
        out = [self.empty((F, ld), torch.int32), self.zeros((F,), torch.int32), *outputs(F, ld)]
        if F and ld:
            need = int(getattr(self.lib, "caelo_%s_ws_bytes" % sym)(F, ld))
            ws = self._ws(sym, need)
            _ffi.check(getattr(self.lib, "caelo_%s_%s" % (sym, entry))(self.ctx, _ptr(pts), F, ld, _ptr(np_d), C.byref(cp), *[_ptr(t) for t in out[2:]],
                                                                      _ptr(out[0]), _ptr(out[1]), _ptr(ws), need, self.stream))
        return [(t[0] if single and t is not None else t) for t in out]

    def iss_keypoints(self, pts, n_pts=None, eig=False, **params):
        """ISS key points on the device (caelo_iss_keypoints, csrc/iss.hip; the definition: include/caelo.h).

        pts [F, ld, 3] f32 (frame f: rows 0 .. n_pts[f]-1; n_pts [F] ints or a device tensor, None = all ld rows) or one cloud
        [n, 3]; params: salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors (caelo.iss.DEFAULTS).
        -> IssKeypoints(key_idx [F, ld] i32: the key points' row indices ascending, -1 behind them; n_key [F] i32; saliency [F, ld]
        f64, -1 where a point is no candidate; eig [F, ld, 3] f64 = e1, e2, e3 and n_neigh [F, ld] i32, the neighbours at
        salient_radius, both None unless ``eig``), on the device; a cloud [n, 3] gives the same without the frame axis.  One all-pairs
        pass for the scatter matrices and one for the suppression: n^2 pair distances each.

        Refused with ValueError before any launch: a non-finite coordinate in a frame's rows (the one read-back of the call; rows past
        n_pts may hold anything), ld above CAELO_ISS_MAX_POINTS, n_pts outside [0, ld], bad parameters (caelo.iss.check_params)."""
        from . import iss
        prm = iss.check_params(**params)
        cp = _ffi.IssParams(prm["salient_radius"], prm["non_max_radius"], prm["gamma_21"], prm["gamma_32"], prm["min_neighbors"], 0)
        return IssKeypoints(*self._detect("iss", "ISS", pts, n_pts, cp, lambda F, ld: (
            self.empty((F, ld), torch.float64), self.empty((F, ld, 3), torch.float64) if eig else None,
            self.empty((F, ld), torch.int32) if eig else None)))

    def harris_keypoints(self, pts, n_pts=None, normals=False, **params):
        """Harris3D key points on the device (caelo_harris_keypoints, csrc/harris.hip; the definition: include/caelo.h).

        pts [F, ld, 3] f32 (frame f: rows 0 .. n_pts[f]-1; n_pts [F] ints or a device tensor, None = all ld rows) or one cloud
        [n, 3]; params: radius, threshold (caelo.harris.DEFAULTS).
        -> HarrisKeypoints(key_idx [F, ld] i32: the key points' row indices ascending, -1 behind them; n_key [F] i32; response [F, ld]
        f64, -1 where a point has no normal; n_neigh [F, ld] i32, the neighbours within radius; normals [F, ld, 3] f64 facing the
        origin, 0 where a point has none -- None unless ``normals``), on the device; a cloud [n, 3] gives the same without the frame
        axis.  Three all-pairs passes (normals, response, suppression): n^2 pair distances each.

        Refused with ValueError before any launch: a non-finite coordinate in a frame's rows (the one read-back of the call; rows past
        n_pts may hold anything), ld above CAELO_ISS_MAX_POINTS, n_pts outside [0, ld], bad parameters (caelo.harris.check_params)."""
        from . import harris
        prm = harris.check_params(**params)
        cp = _ffi.HarrisParams(prm["radius"], prm["threshold"])
        key_idx, n_key, resp, nv, nn = self._detect("harris", "Harris3D", pts, n_pts, cp, lambda F, ld: (
            self.empty((F, ld), torch.float64), self.empty((F, ld, 3), torch.float64) if normals else None,
            self.empty((F, ld), torch.int32)))
        return HarrisKeypoints(key_idx, n_key, resp, nn, nv)

    def sift_octave(self, pts, n_pts=None, sigma=None, min_contrast=0.1, knn=False):
        """One octave of the SIFT3D detector on the device (caelo_sift_octave, csrc/sift.hip; the definition: include/caelo.h,
        DESIGN.md 9j): the difference-of-Gaussians of the points' z over the ascending scales ``sigma`` (3 to 19 of them, float64,
        handed to the kernel as they are), the 25 nearest neighbours, the extremum rule.

        pts [F, ld, 3] f32 (frame f: rows 0 .. n_pts[f]-1; n_pts [F] ints or a device tensor, None = all ld rows) or one cloud [n, 3].
        -> SiftOctave(key_idx [F, ld] i32: the rows with a key at some scale, ascending, -1 behind them; n_key [F] i32; dog [F, ld, S-1]
        f64; knn [F, ld, 25] i32 in (d2, index) order -- None unless ``knn``; key_mask [F, ld] i32, bit s set for a key at sigma[s]),
        on the device; a cloud [n, 3] gives the same without the frame axis.  Two all-pairs passes: n^2 pair distances each.

        Refused with ValueError before any launch: what _detector_frames refuses (a non-finite coordinate in a frame's rows, ld above
        CAELO_ISS_MAX_POINTS, n_pts outside [0, ld]), scales that are not 3 to 19 finite, positive, increasing numbers, a min_contrast
        that is not finite or is negative."""
        from . import sift
        if sigma is None:
            raise ValueError("sift_octave: sigma, the octave's scales, must be given (caelo.sift.octave_scales)")
        sg = sift.check_scales(sigma)
        if isinstance(min_contrast, bool) or not sift._finite(min_contrast) or float(min_contrast) < 0.0:
            raise ValueError("SIFT min_contrast must be finite and not negative (got %r)" % (min_contrast,))
        cp = _ffi.SiftParams(int(sg.shape[0]), 0, float(min_contrast), (C.c_double * _ffi.SIFT_MAX_SCALES)(*sg.tolist()))
        D = int(sg.shape[0]) - 1
        key_idx, n_key, dog, nn, mask = self._detect("sift", "SIFT3D", pts, n_pts, cp, lambda F, ld: (
            self.empty((F, ld, D), torch.float64), self.empty((F, ld, _ffi.SIFT_K), torch.int32) if knn else None,
            self.empty((F, ld), torch.int32)), entry="octave")
        return SiftOctave(key_idx, n_key, dog, nn, mask)

    def voxel_centroids(self, pc, leaf):
        """pc [N, 3] f32 on the device -> [M, 3] f32: the centroids of the occupied ``leaf``-sized cells, cell = floor(double(p) / leaf)
        per component, in (cz, cy, cx) order with x fastest (PCL's VoxelGrid order).  Each coordinate is the float64 sum of the cell's
        points in ascending input row divided by double(count), rounded to float32 (caelo_voxel_centroids: the sort and the run
        detection are torch's, the sums are not -- a scatter-add has no fixed order)."""
        from . import sift
        if not sift._finite(leaf) or not float(leaf) > 0.0:
            raise ValueError("leaf must be finite and positive (got %r)" % (leaf,))
        pc = torch.as_tensor(pc, device=self.device)
        if pc.dim() != 2 or pc.shape[1] != 3 or pc.dtype != torch.float32:
            raise ValueError("pc must be float32 [N, 3], got %s %s" % (pc.dtype, tuple(pc.shape)))
        if not bool(torch.isfinite(pc).all()):
            raise ValueError("voxel_centroids: the cloud holds a non-finite coordinate")
        return self._voxel_centroids_many([pc], float(leaf))[0]

    def _voxel_centroids_many(self, clouds, leaf):
        """voxel_centroids of several clouds ([n_k, 3] f32 on the device, finite) at one leaf -> a list of [m_k, 3] f32: the frame is the
        leading digit of the sort key, so one stable sort, one run detection, one launch and two read-backs serve all of them, and
        every cloud gets what it gets alone (its cells in the same order, each cell's rows in ascending input row)."""
        sizes = [int(c.shape[0]) for c in clouds]
        n = sum(sizes)
        if n == 0:
            return [c.contiguous() for c in clouds]
        pc = (torch.cat(clouds) if len(clouds) > 1 else clouds[0]).contiguous()
        frame = torch.repeat_interleave(torch.arange(len(clouds), device=self.device), torch.tensor(sizes, device=self.device))
        # a device tensor as the divisor: an IEEE division per element (a Python number may be turned into a multiplication)
        cell = torch.floor(pc.to(torch.float64) / torch.tensor(leaf, dtype=torch.float64, device=self.device))
        cell = cell - cell.min(dim=0).values
        ext = cell.max(dim=0).values + 1
        ex, ey, ez = ext.tolist()
        if len(clouds) * ex * ey * ez >= 2.0 ** 62:
            raise ValueError("voxel_centroids: %g-sized cells over this cloud's extent do not fit a 64-bit key" % leaf)
        c, e = cell.to(torch.int64), ext.to(torch.int64)
        key = ((frame * e[2] + c[:, 2]) * e[1] + c[:, 1]) * e[0] + c[:, 0]
        order = torch.argsort(key, stable=True)   # stable: a cell's rows stay in ascending input row
        sk = key[order]
        first = torch.ones_like(sk, dtype=torch.bool)
        first[1:] = sk[1:] != sk[:-1]
        firsts = torch.nonzero(first).reshape(-1)
        starts = torch.cat([firsts, torch.tensor([n], device=self.device)]).to(torch.int32).contiguous()
        m = int(starts.shape[0]) - 1
        out = self.empty((m, 3), torch.float32)
        order32 = order.to(torch.int32).contiguous()
        _ffi.check(self.lib.caelo_voxel_centroids(self.ctx, _ptr(pc), n, _ptr(order32), _ptr(starts), m, _ptr(out), self.stream))
        per = torch.bincount(frame[order[firsts]], minlength=len(clouds)).tolist()   # cells per cloud
        return list(torch.split(out, per))

    def sift_keypoints(self, pts, n_pts=None, details=False, **params):
        """SIFT3D key points on the device: the pyramid of DESIGN.md 9j over sift_octave.  For octave o = 0 .. n_octaves-1 the frame's
        cloud becomes the voxel-grid centroids (voxel_centroids; all frames in one launch) of the previous octave's cloud at leaf min_scale * 2^o (octave 0 starts
        from the given cloud); under 25 points the frame stops; otherwise the octave runs at caelo.sift.octave_scales(min_scale * 2^o,
        n_scales_per_octave), all frames still alive in one call.

        pts [F, ld, 3] f32 with n_pts, or one cloud [n, 3]; params: min_scale, n_octaves, n_scales_per_octave, min_contrast
        (caelo.sift.DEFAULTS).  -> SiftKeypoints(xyz [F, cap, 3] f32: the points of the octave clouds that are a key, in the order
        octave, point index, scale index -- a point may appear more than once; scale [F, cap] f64, the key's sigma; octave [F, cap] i32;
        n_key [F] i32; cap = the largest n_key, rows behind n_key are 0, -1 for octave), on the device, without the frame axis for a
        single cloud.  ``details``: -> (SiftKeypoints, a list per octave of dict(octave, scale, sigma, frames: the frames that ran,
        clouds: their octave clouds, result: the SiftOctave of the batch with knn))."""
        from . import sift
        prm = sift.check_params(**params)
        pts, np_d, single = self._detector_frames(pts, n_pts, "SIFT3D")
        F = int(pts.shape[0])
        counts = np_d.cpu().tolist() if F else []
        clouds = {f: pts[f, :counts[f]] for f in range(F)}
        rows = [[] for _ in range(F)]   # per frame: (xyz [k,3], scale [k], octave [k]) per octave
        octaves = []
        for o in range(prm["n_octaves"]):
            scale = prm["min_scale"] * 2.0 ** o
            alive = sorted(clouds)
            clouds = dict(zip(alive, self._voxel_centroids_many([clouds[f] for f in alive], scale)))   # (finite: _detector_frames checked)
            clouds = {f: c for f, c in clouds.items() if c.shape[0] >= sift.K}
            if not clouds:
                break
            sg = sift.octave_scales(scale, prm["n_scales_per_octave"])
            frames = sorted(clouds)
            sizes = [int(clouds[f].shape[0]) for f in frames]
            ld = max(sizes)
            if ld > sift.MAX_POINTS:
                raise ValueError("SIFT3D: octave %d holds %d points, above the %d an all-pairs search takes (thin the scan first)" % (o, ld, sift.MAX_POINTS))
            batch = self.zeros((len(frames), ld, 3), torch.float32)
            for k, f in enumerate(frames):
                batch[k, :sizes[k]] = clouds[f]
            r = self.sift_octave(batch, n_pts=sizes, sigma=sg, min_contrast=prm["min_contrast"], knn=details)
            sg_d = torch.from_numpy(sg).to(self.device)
            bits = (r.key_mask[:, :, None] >> torch.arange(sg.shape[0], device=self.device, dtype=torch.int32)[None, None, :]) & 1
            hit = torch.nonzero(bits)   # row-major: frame, then point index, then scale index (rows past n_pts have no bit set)
            per = torch.bincount(hit[:, 0], minlength=len(frames)).tolist()
            xyz_o, sc_o, at = batch[hit[:, 0], hit[:, 1]], sg_d[hit[:, 2]], 0
            for k, f in enumerate(frames):
                rows[f].append((xyz_o[at:at + per[k]], sc_o[at:at + per[k]], torch.full((per[k],), o, dtype=torch.int32, device=self.device)))
                at += per[k]
            if details:
                octaves.append(dict(octave=o, scale=scale, sigma=sg, frames=frames, clouds=[clouds[f] for f in frames], result=r))
        n_key = [sum(int(x.shape[0]) for x, _, _ in rows[f]) for f in range(F)]
        cap = max(n_key) if n_key else 0
        xyz = self.zeros((F, cap, 3), torch.float32)
        sc = self.zeros((F, cap), torch.float64)
        oc = torch.full((F, cap), -1, dtype=torch.int32, device=self.device)
        for f in range(F):
            if n_key[f]:
                xyz[f, :n_key[f]] = torch.cat([x for x, _, _ in rows[f]])
                sc[f, :n_key[f]] = torch.cat([s for _, s, _ in rows[f]])
                oc[f, :n_key[f]] = torch.cat([q for _, _, q in rows[f]])
        nk = torch.tensor(n_key, dtype=torch.int32, device=self.device)
        out = SiftKeypoints(xyz[0], sc[0], oc[0], nk[0]) if single else SiftKeypoints(xyz, sc, oc, nk)
        return (out, octaves) if details else out

    def voxelize(self, pc, vmap=None, status=None):
        assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] >= 3 and pc.is_contiguous()
        vmap = vmap or self.voxmap(max(self.max_points, pc.shape[0]))
        status = self.zeros((1,), torch.int32) if status is None else status
        _ffi.check(self.lib.caelo_voxelize(self.ctx, vmap.h, _ptr(pc), pc.shape[0], pc.shape[1], _ptr(status), self.stream))
        return vmap, status

    def voxelize_fast(self, pc, vmap=None, status=None):
        """The one-pass build ``extract`` uses (caelo_voxelize_fast): same voxel sets as ``voxelize``, no first-touch order."""
        assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] >= 3 and pc.is_contiguous()
        vmap = vmap or self.voxmap(max(self.max_points, pc.shape[0]))
        status = self.zeros((1,), torch.int32) if status is None else status
        _ffi.check(self.lib.caelo_voxelize_fast(self.ctx, vmap.h, _ptr(pc), pc.shape[0], pc.shape[1], _ptr(status), self.stream))
        return vmap, status

    def voxmap_voxels(self, vmap, scale, capacity=1 << 18):
        """Voxel set of one scale of a device voxel map -> sorted int32 [n,3] (host; caelo_voxmap_dump, synchronises)."""
        keys = self.empty((capacity,), torch.int64)
        bits = self.empty((capacity, 8), torch.int64)
        count = self.empty((1,), torch.int32)
        _ffi.check(self.lib.caelo_voxmap_dump(self.ctx, vmap.h, int(scale), _ptr(keys), _ptr(bits), capacity, _ptr(count), self.stream))
        n = int(count.item())
        assert n <= capacity, "raise capacity"
        k = keys[:n].cpu().numpy().astype(np.uint64)
        b = np.unpackbits(bits[:n].cpu().numpy().view(np.uint8).reshape(n, 8, 8), axis=2, bitorder="little")  # [brick, x&7, y&7, z&7]
        br, x, y, z = np.nonzero(b.reshape(n, 8, 8, 8))
        base = np.stack([(k >> np.uint64(40)) & np.uint64(0xFFFFF), (k >> np.uint64(20)) & np.uint64(0xFFFFF), k & np.uint64(0xFFFFF)], 1).astype(np.int64) * 8
        vox = (base[br] + np.stack([x, y, z], 1)).astype(np.int32)
        return vox[np.lexsort((vox[:, 2], vox[:, 1], vox[:, 0]))]

    def voxmap_counts(self, vmap):
        """caelo_voxmap_counts: the map's build counters -> int32 [8] (host; synchronises)."""
        out = self.empty((8,), torch.int32)
        _ffi.check(self.lib.caelo_voxmap_counts(self.ctx, vmap.h, _ptr(out), self.stream))
        return out.cpu().numpy()

    def voxmap_export(self, vmap, capacity):
        outs = [self.empty((capacity, 3), torch.int16) for _ in range(3)]
        counts = self.empty((3,), torch.int64)
        _ffi.check(self.lib.caelo_voxmap_export(self.ctx, vmap.h, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                                capacity, _ptr(counts), self.stream))
        n = counts.cpu().tolist()          # (the call itself does not wait for the device; this read does)
        if max(n) > capacity:
            raise _ffi.CaeloError("caelo_voxmap_export: %d voxels exceed the output capacity %d" % (max(n), capacity))
        return [o[:k] for o, k in zip(outs, n)]

    def voxmap_order(self, vmap, scale_mask=7):
        """caelo_voxmap_order: the map (filled by ``voxelize``) records its voxel lists' first-touch order on the device, so that
        ``patches`` on it redoes tie-split patches of the scales in ``scale_mask`` in scikit-learn's kd-tree order.  No sync."""
        _ffi.check(self.lib.caelo_voxmap_order(self.ctx, vmap.h, int(scale_mask), self.stream))
        return vmap

    def voxmap_from_lists(self, a0, a1, a2, vmap=None, status=None):
        for a in (a0, a1, a2):
            assert a.dtype == torch.int16 and a.dim() == 2 and a.shape[1] == 3 and a.is_contiguous()
        vmap = vmap or self.voxmap(max(self.max_points, a0.shape[0], a1.shape[0], a2.shape[0]), slot=1)
        status = self.zeros((1,), torch.int32) if status is None else status
        _ffi.check(self.lib.caelo_voxmap_from_lists(self.ctx, vmap.h, _ptr(a0), a0.shape[0], _ptr(a1), a1.shape[0],
                                                    _ptr(a2), a2.shape[0], _ptr(status), self.stream))
        return vmap, status

    def patches(self, vmap, pts, n_key=None, status=None):
        """-> bits [K,3,64] int64 (bit-packed 16^3 patches), flags [K,3] uint8."""
        assert pts.dtype == torch.float32 and pts.dim() == 2 and pts.shape[1] == 3 and pts.is_contiguous()
        k = pts.shape[0]
        bits = self.empty((k, 3, 64), torch.int64)
        flags = self.empty((k, 3), torch.uint8)
        status = self.zeros((1,), torch.int32) if status is None else status
        _ffi.check(self.lib.caelo_patches(self.ctx, vmap.h, _ptr(pts), k, _ptr(n_key), _ptr(bits), _ptr(flags),
                                          _ptr(status), self.stream))
        return bits, flags

    def patches_many(self, vmaps, pts, n_keys=None, statuses=None):
        """caelo_patches_many: ``patches`` for up to eight maps / key point sets [K,3] of one length K, the kd redo of all of them
        behind one launch of each kd kernel -> ([bits [K,3,64] int64], [flags [K,3] uint8], [status [1] int32]) per map."""
        n, k = len(vmaps), pts[0].shape[0]
        assert 1 <= n <= 8 and len(pts) == n
        for p in pts:
            assert p.dtype == torch.float32 and p.dim() == 2 and p.shape == (k, 3) and p.is_contiguous()
        n_keys = [None] * n if n_keys is None else n_keys
        statuses = [self.zeros((1,), torch.int32) for _ in range(n)] if statuses is None else statuses
        bits = [self.empty((k, 3, 64), torch.int64) for _ in range(n)]
        flags = [self.empty((k, 3), torch.uint8) for _ in range(n)]
        arr = lambda xs: (C.c_void_p * n)(*[x.data_ptr() if x is not None else None for x in xs])
        _ffi.check(self.lib.caelo_patches_many(self.ctx, n, (C.c_void_p * n)(*[m.h for m in vmaps]), arr(pts), k, arr(n_keys), arr(bits),
                                               arr(flags), arr(statuses), self.stream))
        return bits, flags, statuses

    def kd_dump(self, vmap, scale):
        """caelo_voxmap_kd_dump (diagnostic; waits for the stream): the kd-tree of one scale as the last ``patches`` on the map left it
        -> dict(state [32] int32, n, n_nodes, top_levels, idx [n] int32, start / end [n_nodes] int32, lo / hi [n_nodes,3] int16) of NumPy arrays.
        The tree is valid only where ``state[4 + scale] == 1`` (csrc/kdorder.hip)."""
        state = np.zeros(32, np.int32)
        counts = np.zeros(3, np.int64)
        idx_cap, node_cap = int(vmap.max_points), 16384
        idx = np.zeros(idx_cap, np.int32)
        start, end = np.zeros(node_cap, np.int32), np.zeros(node_cap, np.int32)
        lo, hi = np.zeros((node_cap, 3), np.int16), np.zeros((node_cap, 3), np.int16)
        _ffi.check(self.lib.caelo_voxmap_kd_dump(self.ctx, vmap.h, int(scale), _hptr(state), _hptr(idx), idx_cap, _hptr(start), _hptr(end),
                                                 _hptr(lo), _hptr(hi), node_cap, _hptr(counts), self.stream))
        n, nn = int(counts[0]), int(counts[1])
        return dict(state=state, n=n, n_nodes=nn, top_levels=int(counts[2]), idx=idx[:n].copy(), start=start[:nn].copy(), end=end[:nn].copy(), lo=lo[:nn].copy(),
                    hi=hi[:nn].copy())

    def unpack_patches(self, bits):
        n = bits.numel() // 64
        dense = self.empty((n, 16, 16, 16, 1), torch.float32)
        _ffi.check(self.lib.caelo_unpack_patches(self.ctx, _ptr(bits), n, _ptr(dense), self.stream))
        return dense

    def pack_patches(self, dense):
        assert dense.dtype == torch.float32 and dense.is_contiguous()
        n = dense.numel() // 4096
        bits = self.empty((n, 64), torch.int64)
        _ffi.check(self.lib.caelo_pack_patches(self.ctx, _ptr(dense), n, _ptr(bits), self.stream))
        return bits

    def encode(self, bits, group=1):
        """bits [..., 64] int64 -> features [n/group, 20*group] f32."""
        assert bits.dtype == torch.int64 and bits.is_contiguous()
        n = bits.numel() // 64
        assert n % group == 0
        out = self.empty((n // group, 20 * group), torch.float32)
        ws = self._encode_ws(n)
        _ffi.check(self.lib.caelo_encode(self.ctx, _ptr(bits), n, group, _ptr(out), 20 * group, _ptr(ws), self.stream))
        return out

    def decode(self, codes, group=1, target=None, threshold=0.1, prob=False, bits=True, loss=None, counts=None):
        """caelo_decode: codes [m, ld] f32 (contiguous; patch p = row p // group, columns (p % group) * 20 .. + 20: ``group=1`` on
        [n,20] codes, ``group=3`` on the [K,64] descriptor rows of ``extract`` / the pipeline) through the engine's decoder ->
        Decoded(prob [n,4096] f32 in (x, y, z) order, bits [n,64] int64 (voxel set <=> prob > threshold), loss [n] f32 (Keras
        binary_crossentropy against ``target`` [n,64] int64), counts [n,3] int32 (voxels set in target, in bits, in both)); a field
        that was not asked for is None.  ``loss`` / ``counts`` default to "when a target is given".  No host sync."""
        assert codes.dtype == torch.float32 and codes.dim() == 2 and codes.is_contiguous()
        group, ld = int(group), int(codes.shape[1])
        n = codes.shape[0] * group
        if target is not None:
            assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == n * 64, "target: [n, 64] int64"
        loss = target is not None if loss is None else bool(loss)
        counts = target is not None if counts is None else bool(counts)
        out = Decoded(self.empty((n, 4096), torch.float32) if prob else None, self.empty((n, 64), torch.int64) if bits else None,
                      self.empty((n,), torch.float32) if loss else None, self.empty((n, 3), torch.int32) if counts else None)
        if n == 0 and any(o is not None for o in out):   # (an empty tensor has no address to hand over)
            return out
        ws = self._ws("decode", int(self.lib.caelo_decode_ws_bytes(n)))
        _ffi.check(self.lib.caelo_decode(self.ctx, _ptr(codes), n, group, ld, _ptr(target), float(threshold), _ptr(out.prob), _ptr(out.bits),
                                         _ptr(out.loss), _ptr(out.counts), _ptr(ws), self.stream))
        return out

    def decode_layers(self, codes):
        """Test aid: decode [n,20] codes (bits only) and return what Dense(2048) left in the workspace -- G4 [n,2048] f32, activated
        (caelo_decode_ws_layout)."""
        n = codes.shape[0]
        self.decode(codes)
        ws = self._ws("decode", int(self.lib.caelo_decode_ws_bytes(n)))
        lay = (C.c_int64 * 2)()
        _ffi.check(self.lib.caelo_decode_ws_layout(n, C.cast(lay, C.c_void_p)))
        off, rows = int(lay[0]), int(lay[1])
        return ws[off:off + rows * 8192].view(torch.float32).view(rows, 2048).clone()

    def encode_layers(self, bits):
        """Test aid: encode (group 1, every patch) and return the activations the four encoder kernels leave in the
        workspace -- P2 [n,1024] (after pool2), F3 [n,2048] (after conv3), the Dense(200) pre-activations summed over the
        k slices [n,200] (bias not added) -- and the descriptors [n,20].  P2, F3 and the descriptors are activated; to the
        fourth output the caller adds dense_1's bias and applies the model's HIDDEN activation (encoder_activations()[0]: tanh
        or relu).  Workspace layout: caelo_encode_ws_layout."""
        n = bits.numel() // 64
        out = self.encode(bits, 1)
        ws = self._encode_ws(n)
        lay = (C.c_int64 * 6)()
        _ffi.check(self.lib.caelo_encode_ws_layout(n, C.cast(lay, C.c_void_p)))
        o_p2, o_f3, o_part, np_, used, sized = (int(v) for v in lay)
        p2 = ws[o_p2:o_p2 + np_ * 4096].view(torch.float32).view(np_, 1024)[:n]
        f3 = ws[o_f3:o_f3 + np_ * 8192].view(torch.float32).view(np_, 2048)[:n]
        part = ws[o_part:o_part + sized * np_ * 208 * 4].view(torch.float32).view(sized, np_, 208)[:used, :n, :200].sum(dim=0)
        return p2.clone(), f3.clone(), part, out

    # ---- BASELINE.json configs[4]: 32^3 patches (stress case, not a reference code path; csrc/config5.hip) -----
    @staticmethod
    def seeded_dense1_32(seed=5):
        """The stand-in dense_1 of the 32^3 encoder: N(0, 1/16384) [16384,200] f32 and a zero bias (SURVEY.md
        section 7 item 7 -- no trained weights exist at this size)."""
        import numpy as np
        rs = np.random.RandomState(seed)
        return (rs.standard_normal((16384, 200)) / 128.0).astype(np.float32), np.zeros(200, np.float32)

    def set_encoder32_dense(self, wd1, bd1):
        import numpy as np
        wd1 = np.ascontiguousarray(wd1, np.float32)
        bd1 = np.ascontiguousarray(bd1, np.float32)
        assert wd1.shape == (16384, 200) and bd1.shape == (200,)
        _ffi.check(self.lib.caelo_set_encoder32_dense(self.ctx, _hptr(wd1), _hptr(bd1)))

    def patches32(self, vmap, pts, n_key=None):
        """-> bits [K,3,512] int64: bit-packed 32^3 patches, window [-16,16)^3, no 496-NN cap."""
        assert pts.dtype == torch.float32 and pts.dim() == 2 and pts.stride(1) == 1 and pts.shape[1] >= 3
        k = pts.shape[0]
        bits = self.empty((k, 3, 512), torch.int64)
        _ffi.check(self.lib.caelo_patches32(self.ctx, vmap.h, _ptr(pts), int(pts.stride(0)), k, _ptr(n_key), _ptr(bits),
                                            self.stream))
        return bits

    def encode32(self, bits, group=1):
        """bits [..., 512] int64 -> features [n/group, 20*group] f32."""
        assert bits.dtype == torch.int64 and bits.is_contiguous()
        n = bits.numel() // 512
        assert n % group == 0
        out = self.empty((n // group, 20 * group), torch.float32)
        ws = self._ws("encode32", int(self.lib.caelo_encode32_ws_bytes(n)))
        _ffi.check(self.lib.caelo_encode32(self.ctx, _ptr(bits), n, group, _ptr(out), 20 * group, _ptr(ws), self.stream))
        return out

    def encode32_layers(self, bits):
        """Test aid, the counterpart of ``encode_layers``: encode32 (group 1, every patch) and return what its kernels leave in
        the workspace -- P1 [n,16,16,16,8] (after conv1 + pool), P2 [n,8192] (after conv2 + pool), F3 [n,16384] (after conv3), the
        Dense(200) pre-activations summed over the k slices [n,200] (bias not added) -- and the descriptors [n,20].  Workspace
        layout: caelo_encode32_ws_layout."""
        n = bits.numel() // 512
        out = self.encode32(bits, 1)
        ws = self._ws("encode32", int(self.lib.caelo_encode32_ws_bytes(n)))
        lay = (C.c_int64 * 7)()
        _ffi.check(self.lib.caelo_encode32_ws_layout(n, C.cast(lay, C.c_void_p)))
        o_p1, o_p2, o_f3, o_part, np_, used, sized = (int(v) for v in lay)
        p1 = ws[o_p1:o_p1 + n * 32768 * 4].view(torch.float32).view(n, 16, 16, 16, 8)
        p2 = ws[o_p2:o_p2 + n * 8192 * 4].view(torch.float32).view(n, 8192)
        f3 = ws[o_f3:o_f3 + np_ * 16384 * 4].view(torch.float32).view(np_, 16384)[:n]
        part = ws[o_part:o_part + sized * np_ * 208 * 4].view(torch.float32).view(sized, np_, 208)[:used, :n, :200].sum(dim=0)
        return p1.clone(), p2.clone(), f3.clone(), part, out

    def encode32_profile(self, bits, group=1):
        """encode32 + per-launch HIP-event timings (ms): conv1+pool, conv2+pool, conv3, Dense(200)+head.  Synchronises."""
        n = bits.numel() // 512
        out = self.empty((n // group, 20 * group), torch.float32)
        ws = self._ws("encode32", int(self.lib.caelo_encode32_ws_bytes(n)))
        ms = (C.c_float * 4)()
        _ffi.check(self.lib.caelo_encode32_profile(self.ctx, _ptr(bits), n, group, _ptr(out), 20 * group, _ptr(ws), self.stream,
                                                   C.cast(ms, C.c_void_p)))
        return out, list(ms)

    def extract32(self, pc, dist_channels=5):
        """Config-5 frame features: the key points of ``extract`` (project -> response -> top-K rule), described by
        32^3 patches instead of 16^3 ones.  Staged calls; the 16^3 descriptors ``extract`` also produced are
        overwritten in the rows."""
        ff = self.extract(pc, dist_channels, vmap=self.voxmap(max(self.max_points, pc.shape[0])))
        vmap = self.voxmap(max(self.max_points, pc.shape[0]))
        bits = self.patches32(vmap, ff.key_pts, ff.n_key)
        ff.rows[:, 0:60] = self.encode32(bits, group=3)
        return ff

    def encode_profile(self, bits, group=1):
        """encode + per-kernel HIP-event timings (ms): stage1, conv3, dense1, head, then the MFMA instructions stage 1
        executed (millions) and the FLOPs of one of them.  Synchronises."""
        n = bits.numel() // 64
        out = self.empty((n // group, 20 * group), torch.float32)
        ws = self._encode_ws(n)
        ms = (C.c_float * 6)()
        _ffi.check(self.lib.caelo_encode_profile(self.ctx, _ptr(bits), n, group, _ptr(out), 20 * group, _ptr(ws),
                                                 self.stream, C.cast(ms, C.c_void_p)))
        return out, list(ms)

    @staticmethod
    def _ld(t):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
        return int(t.stride(0))

    def match(self, f0, f1, n0=None, n1=None):
        """f0 [k0,dim], f1 [k1,dim] (row-strided views allowed) -> pair_idx [k1] int64."""
        idx = self.zeros((f1.shape[0],), torch.int64)
        kmax, dim = max(int(f0.shape[0]), int(f1.shape[0])), int(f0.shape[1])
        if dim > 64:   # the screen over several K = 64 blocks: one more operand image per block (caelo_match_ws_bytes_dim)
            ws = self._ws("match%d_%d" % (kmax, dim), int(self.lib.caelo_match_ws_bytes_dim(kmax, dim)))
        else:
            ws = self._ws("match%d" % kmax, int(self.lib.caelo_match_ws_bytes(kmax)))   # sized by the larger frame (caelo.h)
        _ffi.check(self.lib.caelo_match(self.ctx, _ptr(f0), self._ld(f0), f0.shape[0], _ptr(n0), _ptr(f1), self._ld(f1),
                                        f1.shape[0], _ptr(n1), f0.shape[1], _ptr(idx), _ptr(ws), self.stream))
        return idx

    def match_profile(self, frames, repeats=20):
        """The pipeline's launch shape of the NN match: len(frames) - 1 pairs of consecutive FrameFeatures behind one k_match_prep +
        one k_match_screen launch, timed with HIP events (caelo_match_profile).  -> (ms both kernels, ms prep alone, pair_idx [n,1024])."""
        n = len(frames) - 1
        assert 1 <= n <= 8 and all(f.rows.is_contiguous() for f in frames)
        rows = (C.c_void_p * (n + 1))(*[f.rows.data_ptr() for f in frames])
        nk = (C.c_void_p * (n + 1))(*[f.n_key.data_ptr() for f in frames])
        idx = self.zeros((n, MAX_K), torch.int64)
        ws = self._ws("match_profile", n * int(self.lib.caelo_match_ws_bytes(MAX_K)))
        ms = (C.c_float * 2)()
        _ffi.check(self.lib.caelo_match_profile(self.ctx, rows, n, nk, _ptr(idx), _ptr(ws), int(repeats), self.stream, C.cast(ms, C.c_void_p)))
        return float(ms[0]), float(ms[1]), idx

    def solve_rt(self, p0, p1):
        assert p0.shape == p1.shape and p0.dtype == torch.float32 and p0.is_contiguous() and p1.is_contiguous()
        R = self.empty((3, 3), torch.float32)
        T = self.empty((3, 1), torch.float32)
        cred = self.empty((1,), torch.int32)
        _ffi.check(self.lib.caelo_solve_rt(self.ctx, _ptr(p0), _ptr(p1), p0.shape[0], _ptr(R), _ptr(T), _ptr(cred), self.stream))
        return R, T, cred

    def ransac(self, pc0, pc1, pair_idx, rand, n1=None, cert=None):
        """rand: [1500,4] f64 uniform draws (device).  -> (result bytes tensor, mask [k1] uint8).  ``cert``: a
        [sizeof(caelo_ransac_cert)] u8 device tensor that receives the pair's certificate (``new_cert``)."""
        assert pair_idx.dtype == torch.int64 and pair_idx.is_contiguous()
        assert rand.dtype == torch.float64 and rand.numel() >= 6000 and rand.is_contiguous()
        res = self.empty((C.sizeof(_ffi.PoseResult),), torch.uint8)
        mask = self.empty((pc1.shape[0],), torch.uint8)
        _ffi.check(self.lib.caelo_ransac(self.ctx, _ptr(pc0), self._ld(pc0), _ptr(pc1), self._ld(pc1), _ptr(pair_idx),
                                         pc1.shape[0], _ptr(n1), _ptr(rand), _ptr(res), _ptr(mask),
                                         _ptr(self._ws("ransac", self.lib.caelo_ransac_ws_bytes())), _ptr(cert), self.stream))
        return res, mask

    def new_cert(self, k=1):
        """k zeroed caelo_ransac_cert records on the device."""
        return self.zeros((k, _ffi.CERT_DTYPE.itemsize), torch.uint8)

    # ---- the host half of the exact RANSAC (csrc/certify.hip, caelo/hostexact.py) ------------------------------------
    def bound_violations(self):
        """caelo_host_bound_violations: exact hypothesis counts the host half found above the device's upper bound since the process
        started (such a pair is decided by the reference's loop without bounds: still exact).  0 on every run so far."""
        return int(self.lib.caelo_host_bound_violations())

    def host_blas(self):
        """Bind libcaelo's host half to the BLAS / LAPACK of this process's NumPy (once; caelo/hostblas.py)."""
        from . import hostblas
        return hostblas.bind(self.lib)

    def certify(self, certs, rands=None, threads=None):
        """certs: [k, sizeof(caelo_ransac_cert)] u8 device tensor.  Copies the records to the host (synchronises) and runs
        caelo_host_certify: Match.py:181-214 replayed over the device's bounds, the deciding hypotheses re-evaluated through
        NumPy's own BLAS / LAPACK entry points.  ``rands``: the pairs' draws (list of host arrays or device tensors, or None) --
        only read for a pair that escalates beyond the 0.4 m level.  -> (results record array [k] (_ffi.POSE_DTYPE),
        masks [k,1024] u8, evals [k] i32, status [k] i32: 0 exact, 2 no bounds in the record (> 1024 pairs), 3 no record)."""
        k = int(certs.shape[0])
        nb = _ffi.CERT_DTYPE.itemsize
        assert certs.dtype == torch.uint8 and certs.dim() == 2 and certs.shape[1] == nb and certs.is_contiguous()
        host = self._pinned("cert", k * nb)[:k * nb].view(k, nb)
        host.copy_(certs, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        from . import hostexact
        return hostexact.certify_records(host.numpy(), rands, threads)

    def certify_batch(self, out, rands=None, threads=None):
        """Engine.certify over a FrameBatch that ran with ``certify=True``: the exact results replace ``out.result`` /
        ``out.inlier_mask`` on the device (frames without a pair keep what they had) and stay on the host in ``out.exact`` =
        (results, masks, evals, status).  Synchronises."""
        assert out.cert is not None, "run the pipeline with certify=True"
        res, masks, evals, status = self.certify(out.cert[:out.k], rands, threads)
        ok = status == 0
        if (status == 2).any():
            raise _ffi.CaeloError("a pair holds more than 1024 matches: no certificate (use api.RANSAC4RT for such inputs)")
        if ok.all():
            out.result[:out.k].copy_(torch.from_numpy(res.view(np.uint8).reshape(out.k, -1)), non_blocking=False)
            out.inlier_mask[:out.k].copy_(torch.from_numpy(masks), non_blocking=False)
        elif ok.any():
            sel = torch.from_numpy(np.flatnonzero(ok)).to(self.device)
            out.result[sel] = torch.from_numpy(np.ascontiguousarray(res.view(np.uint8).reshape(out.k, -1)[ok])).to(self.device)
            out.inlier_mask[sel] = torch.from_numpy(np.ascontiguousarray(masks[ok])).to(self.device)
        out.exact = (res, masks, evals, status)
        return out.exact

    def _pinned(self, kind, nbytes):
        t = self._pin.get(kind) if hasattr(self, "_pin") else None
        if t is None or t.numel() < nbytes:
            if not hasattr(self, "_pin"):
                self._pin = {}
            t = self._pin[kind] = torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True)
        return t

    @staticmethod
    def pose_result(res):
        """Synchronising read of a caelo_pose_result."""
        return _ffi.PoseResult.from_buffer_copy(res.cpu().numpy().tobytes())

    # ---- fused hot path ------------------------------------------------------------------------------
    def extract(self, pc, dist_channels=5, vmap=None, rows=None, exact_voxels=False, dedup=True, exact_patches=False, key_pts=None,
                calib_angle=None):
        """scan [N,4] f32 (device) -> FrameFeatures, ONE C-ABI call (caelo_extract), no host sync:
        project -> response CNN -> keypoints -> voxelize -> patch gather -> 3x encoder.
        dist_channels: 5 = demo calling mode (SphericalRing.py:414), 3 = batch mode
        (BatchPreprocess.py:97-98,131-136).  ``rows``: optional [1024,64] f32 output slot.
        The default one-pass voxelization and ``exact_voxels=True`` (the two-pass first-touch kernels of
        ``voxelize``, Voxel.py:139-141) produce the same voxel sets on every cloud, points on voxel faces
        included (metrically quantised scans have some in every frame).  ``dedup=False`` encodes
        every patch even when it is a bit-identical copy of another one of the frame (same result, more work).
        ``exact_patches=True``: GetPatchesList's patches where the 496-nearest cut splits a class of equidistant voxels too (the
        canonical rule's patches are redone on the device in the library's order before the encoder runs, flags & 4) -- what
        ``extract`` + ``resolve_ties`` give, in the same single call.  ``status[0]`` may carry ST_TIES_LEFT (see ``note_ties_left``).
        ``key_pts``: [K,3] f32 key points of another source (CAELO_EXTRACT_GIVEN_KEYPTS: GetPatchesList + GetFeaturesFromPatches on
        them, PoseEstimation.py:26-45) instead of the detector's; K in [1, 1024] and |x|, |y|, |z| <= 16384 m, checked on the device
        (``status[0]`` & ST_BAD_KEYPTS, raised by ``raise_status`` as ValueError).  ``key_pixels`` are then -1.
        ``calib_angle``: degrees; the scan is first corrected by the reference's CorrectPC (CAELO_EXTRACT_CORRECT_PC: sets the
        context's angle and the mode bit) into storage of the voxel map, inside the same call -- ``extract(correct_pc(pc, a))`` bit
        for bit; ``pc`` is not written and given key points are not corrected.  A scan with a point on the z axis then reports
        ST_NONFINITE (the reference's NaN)."""
        assert pc.dtype == torch.float32 and pc.dim() == 2 and pc.shape[1] == 4 and pc.is_contiguous()
        ws = self._ws("extract", int(self.lib.caelo_extract_ws_bytes()))
        vmap = vmap or self.voxmap(max(self.max_points, pc.shape[0]))
        if calib_angle is not None:
            self.set_calib_angle(calib_angle)
        rows = self.empty((MAX_K, 64), torch.float32) if rows is None else rows
        assert rows.shape == (MAX_K, 64) and rows.is_contiguous()
        kpix = self.empty((MAX_K, 2), torch.int64)
        nkey = self.empty((1,), torch.int32)
        if key_pts is not None:   # (more than 1024 rows: the first 1024 are copied, the count tells the device to refuse them)
            kp = _given_pts(self, key_pts)
            rows[:min(kp.shape[0], MAX_K), 60:63] = kp[:MAX_K]
            nkey.fill_(kp.shape[0])
        flags = self.empty((MAX_K, 3), torch.uint8)
        status = self.empty((4,), torch.int32)
        base = rows.data_ptr()
        _ffi.check(self.lib.caelo_extract(self.ctx, vmap.h, _ptr(pc), pc.shape[0], dist_channels,
                                          extract_mode(exact_voxels, dedup, exact_patches, key_pts is not None, correct_pc=calib_angle is not None),
                                          C.c_void_p(base + 240), 64, C.c_void_p(base), 64, C.c_void_p(base + 252), 64,
                                          _ptr(kpix), _ptr(nkey), _ptr(flags), _ptr(status), _ptr(ws),
                                          self.stream))
        return FrameFeatures(rows, kpix, nkey, status, flags)

    def extract_frame_tables(self):
        """Test aid: what the last ``extract`` on the current stream left in its workspace (caelo_extract_ws_frame_offset) -> host
        arrays (bits [3072,64] uint64, the patches by key point * 3 + scale; count; list [3072] int32; slot_of [3072] int32) of
        csrc/dedup.hip's caelo_dedup_tables.  Synchronises."""
        ws = self._ws("extract", int(self.lib.caelo_extract_ws_bytes()))
        off, n = int(self.lib.caelo_extract_ws_frame_offset()), 3 * MAX_K
        torch.cuda.current_stream(self.device).synchronize()
        raw = ws[off:off + n * 512 + 256 + 8 * n].cpu().numpy()
        tab = raw[n * 512:].view(np.int32)
        return raw[:n * 512].view(np.uint64).reshape(n, 64), int(tab[0]), tab[64:64 + n].copy(), tab[64 + n:64 + 2 * n].copy()

    def extract_kp_eligible(self):
        """Test aid: the key point eligibility map the last ``extract`` on the current stream left in its workspace
        (caelo_extract_ws_kp_eligible_offset) -> host array [64] uint64, bit b of word y = some pixel of columns 32 b .. 32 b + 31
        of ring row y passes the rule's range gate.  Synchronises."""
        ws = self._ws("extract", int(self.lib.caelo_extract_ws_bytes()))
        off = int(self.lib.caelo_extract_ws_kp_eligible_offset())
        torch.cuda.current_stream(self.device).synchronize()
        return ws[off:off + 512].cpu().numpy().view(np.uint64).copy()

    def extract_patch_bits(self):
        """The bit-packed patches the last ``extract`` on the current stream gathered -> [1024,3,64] int64 (device, a copy; rows past
        ``n_key`` are not meaningful).  No host sync."""
        ws = self._ws("extract", int(self.lib.caelo_extract_ws_bytes()))
        off, n = int(self.lib.caelo_extract_ws_frame_offset()), 3 * MAX_K
        return ws[off:off + n * 512].view(torch.int64).view(MAX_K, 3, 64).clone()

    def resolve_ties(self, ff, pc):
        """The fused path (extract / Pipeline.run) builds voxel SETS; where the 496-nearest cut of Voxel.py:195-196 splits a class
        of equidistant voxels it uses a canonical rule and sets flag bit 2, because scikit-learn's choice depends on the ORDER of
        the voxel lists.  This redoes such a frame's patches the reference's way -- the exact voxelization (caelo_voxelize: first
        touch recorded), the lists of the scales that need it ordered on the device (caelo_voxmap_order), caelo_patches with the
        kd-tree order (kdorder.hip), caelo_encode -- and writes the descriptors into ``ff.rows`` in place.  Synchronises; returns
        the number of tie-split patches it found (0: nothing done).  Rare: 0 of 614 400 patches on the KITTI-shaped scene, 115 on
        the clutter scene.  Many frames at once: ``resolve_ties_many``."""
        per = ((ff.flags & 2) != 0).sum(dim=0).cpu().tolist()          # tie-split patches per scale
        n_tie = int(sum(per))
        if n_tie == 0:
            return 0
        cap = max(self.max_points, pc.shape[0])
        vm, st = self.voxelize(pc, self.voxmap(cap, slot=2))
        self.voxmap_order(vm, sum(1 << s_ for s_ in range(3) if per[s_]))
        k = int(ff.n_key.item())
        bits, flags = self.patches(vm, ff.key_pts[:k].contiguous())
        raise_status(int(st.item()))
        ff.rows[:k, 0:60] = self.encode(bits.reshape(-1, 64), group=3)
        ff.flags[:k] = flags
        return n_tie

    def resolve_ties_many(self, items, lanes=8, batch=None):
        """resolve_ties over many frames at once: ``items`` = [(FrameFeatures, scan), ...] (``batch``: the FrameBatch whose frames
        0 .. len(items) - 1 they are, if so).  One read of the flags and key point counts for all of them, then each tied frame's
        redo is issued -- without any further host read -- to one of ``lanes`` side streams (own voxel maps and scratch per stream),
        so the kd-tree builds and queries of different frames, a few workgroups each, overlap instead of queueing (more lanes than
        hardware queues, 8, buy nothing).  The current stream waits for the lanes; one read of the status words at the end.
        -> (indices into ``items`` that were redone, their numbers of tie-split patches)."""
        t0_ = time.perf_counter()
        if not items:
            return [], []
        if batch is not None:          # the frames are frames 0 .. len(items) - 1 of a FrameBatch: two reductions instead of two per frame
            tie = ((batch.flags[:len(items)] & 2) != 0).sum(dim=1)
            nk = batch.n_key[:len(items)].reshape(-1)
        else:
            tie = torch.stack([((ff.flags & 2) != 0).sum(dim=0) for ff, _ in items])      # [frames, 3 scales]
            nk = torch.stack([ff.n_key.reshape(()) for ff, _ in items])
        both = torch.cat([tie.to(torch.int64), nk.to(torch.int64).reshape(-1, 1)], dim=1).cpu().numpy()
        tied = [i for i in range(len(items)) if both[i, :3].any()]
        if not tied:
            return [], []
        if not hasattr(self, "_tie_lanes") or len(self._tie_lanes) < lanes:
            self._tie_lanes = [torch.cuda.Stream(self.device) for _ in range(lanes)]
        cur = torch.cuda.current_stream(self.device)
        start = torch.cuda.Event()
        start.record(cur)
        t1_ = time.perf_counter()
        statuses = []
        # Groups of up to eight tied frames per side stream (round 6): each frame's exact voxelization and list ordering one after the
        # other, then ONE caelo_patches_many -- the kd-tree builds and queries of the whole group behind one launch of each kd kernel
        # (a redo's chain of ~150 dependent quickselect passes costs a millisecond or two whatever the GPU has free: eight side by side
        # cost what one does) -- and ONE encoder launch set over the group's patches.  Frame by frame on eight lanes this took 1.2 ms per
        # tied frame (profiles/r05_ties_many.txt, r06_ties_many.txt).
        G = 8
        groups = [tied[g0:g0 + G] for g0 in range(0, len(tied), G)]
        n_lanes = min(lanes, len(groups))
        for gi, grp in enumerate(groups):
            lane = self._tie_lanes[gi % lanes]
            if gi < lanes:
                lane.wait_event(start)
            with torch.cuda.stream(lane):
                n = len(grp)
                gbits = self.empty((n, MAX_K, 3, 64), torch.int64)
                gflags = self.empty((n, MAX_K, 3), torch.uint8)
                gpts = self.empty((n, MAX_K, 3), torch.float32)
                maps, sts = [], []
                for q, i in enumerate(grp):
                    ff, pc = items[i]
                    cap = max(self.max_points, pc.shape[0])
                    vm, st = self.voxelize(pc, self.voxmap(cap, slot=10 + q))      # exact build: first touch recorded
                    self.voxmap_order(vm, sum(1 << s_ for s_ in range(3) if both[i, s_]))
                    gpts[q].copy_(ff.key_pts)
                    maps.append(vm)
                    sts.append(st)
                    statuses.append(st)
                arr = lambda xs: (C.c_void_p * n)(*xs)
                _ffi.check(self.lib.caelo_patches_many(self.ctx, n, arr([m.h for m in maps]), arr([gpts[q].data_ptr() for q in range(n)]), MAX_K,
                                                       arr([items[i][0].n_key.data_ptr() for i in grp]), arr([gbits[q].data_ptr() for q in range(n)]),
                                                       arr([gflags[q].data_ptr() for q in range(n)]), arr([st.data_ptr() for st in sts]), self.stream))
                feats = self.encode(gbits.reshape(-1, 64), group=3).reshape(n, MAX_K, 60)
                for q, i in enumerate(grp):
                    ff = items[i][0]
                    k = int(both[i, 3])
                    ff.rows[:k, 0:60] = feats[q, :k]
                    ff.flags[:k] = gflags[q, :k]
                for t in (gbits, gflags, gpts, feats):
                    t.record_stream(lane)
        for lane in self._tie_lanes[:n_lanes]:
            cur.wait_stream(lane)
        t4_ = time.perf_counter()
        raise_status(int(np.bitwise_or.reduce(torch.stack([s.reshape(()) for s in statuses]).cpu().numpy())))
        # a redone patch carries flag 4 instead of 2 (kdorder.hip); one that still carries 2 on a list long enough for the library's
        # kd-tree was LEFT on the canonical rule (the tree build gave up on a quickselect): not the reference's patch -- say so
        left = int(torch.stack([((items[i][0].flags[:int(both[i, 3])] & 2) != 0).sum() for i in tied]).sum().item())
        self.last_tie_unresolved = left
        if left:
            import warnings
            warnings.warn("%d tie-split patch(es) were left on the canonical rule by the kd-tree redo (flag 2 still set)" % left)
        t5_ = time.perf_counter()
        self.last_tie_times = dict(find_ms=1e3 * (t1_ - t0_), issue_ms=1e3 * (t4_ - t1_), wait_ms=1e3 * (t5_ - t4_))
        return tied, [int(both[i, :3].sum()) for i in tied]

    def match_pose_exact_many(self, pairs, rands, rands_host=None, threads=None, lanes=8):
        """match_pose_exact over many pairs [(fa, fb), ...]: every match and hypothesis launch is issued first, the certificates
        come back in one copy and the host half runs over them on ``threads`` threads.  -> (results [k] (_ffi.POSE_DTYPE),
        masks [k,1024] u8 (host), [pair_idx (device)] * k).  Synchronises once."""
        k = len(pairs)
        cur = torch.cuda.current_stream(self.device)
        cert = self.new_cert(k)
        idxs = []
        # pair j goes to side stream j % lanes (match and hypothesis kernels of one pair are ~0.1 ms of dependent launches that
        # leave most of the GPU idle; the workspaces are per stream)
        lanes = min(int(lanes), k)
        if lanes > 1:
            if not hasattr(self, "_tie_lanes") or len(self._tie_lanes) < lanes:
                self._tie_lanes = [torch.cuda.Stream(self.device) for _ in range(max(lanes, 8))]
            start = torch.cuda.Event()
            start.record(cur)
        for j, (fa, fb) in enumerate(pairs):
            s_ = self._tie_lanes[j % lanes] if lanes > 1 else cur
            if lanes > 1 and j < lanes:
                s_.wait_event(start)
            for f in (fa, fb):
                f.rows.record_stream(s_)
                f.n_key.record_stream(s_)
            with torch.cuda.stream(s_):
                idx = self.match(fa.features, fb.features, fa.n_key, fb.n_key)
                res_, mask_ = self.ransac(fa.key_pts, fb.key_pts, idx, rands[j], fb.n_key, cert=cert[j])
            for t in (idx, res_, mask_):
                t.record_stream(cur)
            idxs.append(idx)
        if lanes > 1:
            for s_ in self._tie_lanes[:lanes]:
                cur.wait_stream(s_)
        results, masks, _, status = self.certify(cert, list(rands_host) if rands_host is not None else list(rands), threads)
        if (status != 0).any():
            raise _ffi.CaeloError("pairs %s could not be certified (status %s)" % (np.flatnonzero(status != 0).tolist(), status[status != 0].tolist()))
        return results, masks, idxs

    def redo_ties(self, batch, k, scan, draws, prev=None, certify=True):
        """The host redo of a strict-ties run: frames 0 .. k - 1 of ``batch`` (just returned by a pipeline) whose 496-nearest cut
        (Voxel.py:195-196) split a class of equidistant voxels are redone in scikit-learn's kd-tree order (``resolve_ties_many``), then
        the pairs (j - 1, j) such a frame is part of are matched again -- (-1, 0) against ``prev`` when given -- with
        ``match_pose_exact_many`` (``certify``) or ``match_pose``.  ``scan(j)`` -> frame j's scan (device tensor), asked for a tied frame
        only; ``draws(j)`` -> pair j's RANSAC draws (device tensor, host float64 array).  The new results go wherever the run's results
        live: ``result`` / ``inlier_mask`` / ``pair_idx`` on the device and ``batch.exact`` when the run has one.  One host read when
        no frame is tied (the usual case: none on KITTI-shaped scans).  -> (indices of the redone frames, their tie-split patches)."""
        if not bool((batch.flags[:k] & 2).any().item()):
            return [], []
        tied_frames = (batch.flags[:k] & 2).reshape(k, -1).any(dim=1).cpu().numpy()
        tied, counts = self.resolve_ties_many([(batch.frame(j), scan(j) if tied_frames[j] else None) for j in range(k)], batch=batch)
        redo = sorted({t for u in tied for t in (u, u + 1) if t < k and (t > 0 or prev is not None)})
        if not redo:
            return tied, counts
        pairs = [(prev if j == 0 else batch.frame(j - 1), batch.frame(j)) for j in redo]
        rands, rands_host = zip(*[draws(j) for j in redo])
        if certify:
            rs, ms, xs = self.match_pose_exact_many(pairs, rands, rands_host)
            sel = torch.tensor(redo, device=self.device)
            batch.result[sel] = torch.from_numpy(rs.view(np.uint8).reshape(len(redo), -1).copy()).to(self.device)
            batch.inlier_mask[sel] = torch.from_numpy(ms).to(self.device)
            for j, x in zip(redo, xs):
                batch.pair_idx[j].copy_(x)
            if batch.exact is not None:
                batch.exact[0][redo] = rs
                batch.exact[1][redo] = ms
        else:
            for j, (fa, fb), rand in zip(redo, pairs, rands):
                r, m, x = self.match_pose(fa, fb, rand)
                batch.result[j].copy_(r); batch.inlier_mask[j].copy_(m); batch.pair_idx[j].copy_(x)
        return tied, counts

    def _table_args(self, who, rows, n_key, table, desc):
        """What register_pairs and register_pairs_adaptive check alike: rows [F,1024,64], n_key [F], desc [F,1024,D] or None.
        -> the table as [P,2] int64, every index within 32 bits."""
        assert rows.dtype == torch.float32 and rows.dim() == 3 and tuple(rows.shape[1:]) == (MAX_K, 64) and rows.is_contiguous()
        if desc is not None:
            if desc.dtype != torch.float32 or desc.dim() != 3 or tuple(desc.shape[:2]) != (rows.shape[0], MAX_K) or not 1 <= desc.shape[2] <= 256:
                raise ValueError("desc [F=%d,%d,D<=256] f32, got %s %s" % (rows.shape[0], MAX_K, tuple(desc.shape), desc.dtype))
            if desc.stride(2) != 1 or desc.stride(0) != MAX_K * desc.stride(1) or desc.stride(1) < desc.shape[2]:
                raise ValueError("desc must be contiguous or a column slice of a contiguous [F,%d,ld] block, got strides %s" % (MAX_K, tuple(desc.stride())))
        assert n_key.dtype == torch.int32 and n_key.is_contiguous() and n_key.numel() == rows.shape[0]
        pr = np.ascontiguousarray(table.cpu().numpy() if isinstance(table, torch.Tensor) else table, dtype=np.int64).reshape(-1, 2)
        if pr.size and (pr.min() < -(1 << 31) or pr.max() >= (1 << 31)):
            raise _ffi.CaeloError("%s: a frame index does not fit 32 bits" % who)
        return pr

    def register_pairs(self, rows, n_key, pairs, seeds, certify=True, desc=None):
        """The pipeline's pair stage over a table of frame pairs of resident rows, ONE call (caelo_register_pairs): ``rows``
        [F,1024,64] f32 and ``n_key`` [F] i32 on the device (a FrameBatch's), ``pairs`` [P,2] (frame 0, frame 1) -- any two frames,
        (f, f) included -- ``seeds`` one integer per pair (the pair draws ``ransac_draws(seed)``, as the pipeline's pair with that
        seed does) or a float64 array [P,6000] of draws.  ``certify=True``: the kernels leave certificates and the host half runs
        over them as for a pipeline batch (the reference's inlier sets, R_star / T_star and refits, bit for bit); without it the
        kernels' own float64 fits are returned.  -> RegisteredPairs(results [P] (_ffi.POSE_DTYPE: R, T, R_ransac, T_ransac,
        threshold, success, iterations, n_inliers, ...), masks [P,1024] u8 (host), pair_idx [P,1024] i64 (device), evals [P],
        status [P]) in the table's order.  Raises before any launch for a frame index outside [0, F) or a frame of the table whose
        n_key lies outside [1, 1024].  Synchronises.
        ``desc`` [F,1024,D] f32 on the device (D <= 256; contiguous or row-strided, i.e. a column slice of a wider block): the NN
        match runs on these descriptors instead of the rows' columns 0:60 (caelo_register_pairs_desc); the rows still give xyz."""
        pr = self._table_args("register_pairs", rows, n_key, pairs, desc)
        P = int(pr.shape[0])
        if isinstance(seeds, np.ndarray) and seeds.dtype == np.float64:
            draws = np.ascontiguousarray(seeds).reshape(P, -1)
        else:
            assert len(seeds) == P, "one seed per pair"
            draws = np.stack([ransac_draws(int(s_)) for s_ in seeds]) if P else np.zeros((0, 6000))
        assert draws.shape[1] == 6000, "[P,6000] draws: 3 levels x 500 trials x 4"
        pr_d = torch.from_numpy(pr.astype(np.int32)).to(self.device)
        rand_d = torch.from_numpy(draws).to(self.device)
        idx = self.zeros((P, MAX_K), torch.int64)
        if desc is None:
            ws = self._ws("register_pairs", int(self.lib.caelo_register_pairs_ws_bytes(P)))
        else:
            ws = self._ws("register_pairs_d%d" % desc.shape[2], int(self.lib.caelo_register_pairs_ws_bytes_dim(P, int(desc.shape[2]))))
        if certify:
            self.host_blas()
            cert = self.new_cert(P)
            res_d = mask_d = None
        else:
            cert = None
            res_d = self.zeros((P, C.sizeof(_ffi.PoseResult)), torch.uint8)
            mask_d = self.zeros((P, MAX_K), torch.uint8)
        if desc is None:
            _ffi.check(self.lib.caelo_register_pairs(self.ctx, _ptr(rows), rows.shape[0], _ptr(n_key), _ptr(pr_d), P, _ptr(rand_d), _ptr(idx),
                                                     _ptr(res_d), _ptr(mask_d), _ptr(cert), _ptr(ws), self.stream))
        else:
            _ffi.check(self.lib.caelo_register_pairs_desc(self.ctx, _ptr(rows), rows.shape[0], _ptr(n_key), _ptr(pr_d), P, _ptr(rand_d), _ptr(idx),
                                                          _ptr(res_d), _ptr(mask_d), _ptr(cert), _ptr(ws), self.stream,
                                                          _ptr(desc), int(desc.stride(1)), int(desc.shape[2])))
        if P == 0:
            return RegisteredPairs(np.zeros(0, dtype=_ffi.POSE_DTYPE), np.zeros((0, MAX_K), dtype=np.uint8), idx, np.zeros(0, np.int32), np.zeros(0, np.int32))
        if certify:
            results, masks, evals, status = self.certify(cert, list(draws))
            if (status != 0).any():
                raise _ffi.CaeloError("pairs %s could not be certified (status %s)" % (np.flatnonzero(status != 0).tolist(), status[status != 0].tolist()))
            results, masks = results.copy(), masks.copy()
        else:
            results = np.frombuffer(res_d.cpu().numpy().tobytes(), dtype=_ffi.POSE_DTYPE).copy()
            masks = mask_d.cpu().numpy()
            evals, status = np.zeros(P, np.int32), np.zeros(P, np.int32)
        return RegisteredPairs(results, masks, idx, evals, status)

    # ---- the comparison protocol's registrar (csrc/adaptive.hip, caelo/adaptive.py) ----------------------
    def _adaptive_draws(self, draws):
        if isinstance(draws, torch.Tensor):
            assert draws.dtype == torch.float64 and tuple(draws.shape) == (_ffi.ADAPTIVE_DRAWS, 3) and draws.is_contiguous() and draws.device == self.device
            return draws
        from . import adaptive
        return torch.from_numpy(adaptive.check_draws(draws)).to(self.device)

    def ransac_adaptive(self, x1, x2, draws, threshold=1.0):
        """ransacfitRt.m on the device (caelo_ransac_adaptive): x1, x2 [n, 3] float64 with x1 ~ R x2 + T (host arrays, or device
        tensors), n <= 1024; ``draws`` [10001, 3] f64 (caelo.adaptive.draw_table; host array or device tensor).  One workgroup.
        -> (record (_ffi.ADAPTIVE_DTYPE: R, T the refit, R_ransac, T_ransac the best trial, n_pairs, n_inliers, trials, best_trial,
        status 0 ok / 1 trial limit / 2 fewer than 3 pairs), mask [n] u8 (host)).  Synchronises."""
        if isinstance(x1, torch.Tensor):
            a, b = x1, x2
            assert a.dtype == b.dtype == torch.float64 and a.shape == b.shape and a.dim() == 2 and a.shape[1] == 3 and a.is_contiguous() and b.is_contiguous()
            if a.shape[0] > MAX_K:
                raise ValueError("at most %d pairs, got %d" % (MAX_K, a.shape[0]))
        else:
            from . import adaptive
            a, b = (torch.from_numpy(t).to(self.device) for t in adaptive.check_pairs(x1, x2))
        n = int(a.shape[0])
        res = self.zeros((_ffi.ADAPTIVE_DTYPE.itemsize,), torch.uint8)
        mask = self.zeros((max(n, 1),), torch.uint8)
        _ffi.check(self.lib.caelo_ransac_adaptive(self.ctx, _ptr(a), _ptr(b), n, _ptr(self._adaptive_draws(draws)), float(threshold),
                                                  _ptr(res), _ptr(mask), None, self.stream))
        return np.frombuffer(res.cpu().numpy().tobytes(), dtype=_ffi.ADAPTIVE_DTYPE)[0], mask.cpu().numpy()[:n]

    def register_pairs_adaptive(self, rows, n_key, table, draws, threshold=1.0, desc=None):
        """The comparison protocol's registrar over a table of frame pairs of resident rows, ONE call
        (caelo_register_pairs_adaptive): ``rows`` / ``n_key`` / ``desc`` as for ``register_pairs``, ``table`` [P,2] (frame a, frame b),
        ``draws`` [10001, 3] f64 shared by every pair (caelo.adaptive.draw_table).  The match direction is the script's: for each key
        point of frame a the nearest descriptor of frame b -- ``pair_idx`` [P,1024] indexes frame B and ``masks`` [P,1024] is over
        frame A's points, the other way round from ``register_pairs``; the pose maps frame b into frame a all the same.
        -> RegisteredPairs(results [P] (_ffi.ADAPTIVE_DTYPE), masks [P,1024] u8 (host), pair_idx (device), evals = the trial counts,
        status [P]) in the table's order.  The same refusals before any launch as ``register_pairs``.  Synchronises."""
        pr = self._table_args("register_pairs_adaptive", rows, n_key, table, desc)
        P = int(pr.shape[0])
        dim = 60 if desc is None else int(desc.shape[2])
        idx = self.zeros((P, MAX_K), torch.int64)
        if P == 0:   # (an empty tensor has no address to hand to the library)
            return RegisteredPairs(np.zeros(0, dtype=_ffi.ADAPTIVE_DTYPE), np.zeros((0, MAX_K), dtype=np.uint8), idx, np.zeros(0, np.int32), np.zeros(0, np.int32))
        pr_d = torch.from_numpy(pr.astype(np.int32)).to(self.device)
        res_d = self.zeros((P, _ffi.ADAPTIVE_DTYPE.itemsize), torch.uint8)
        mask_d = self.zeros((P, MAX_K), torch.uint8)
        ws = self._ws("register_pairs_adaptive_d%d" % dim, int(self.lib.caelo_register_pairs_adaptive_ws_bytes(P, dim)))
        _ffi.check(self.lib.caelo_register_pairs_adaptive(self.ctx, _ptr(rows), rows.shape[0], _ptr(n_key), _ptr(pr_d), P, _ptr(self._adaptive_draws(draws)),
                                                          float(threshold), _ptr(idx), _ptr(res_d), _ptr(mask_d), _ptr(ws), self.stream,
                                                          _ptr(desc), int(desc.stride(1)) if desc is not None else 64, dim))
        results = np.frombuffer(res_d.cpu().numpy().tobytes(), dtype=_ffi.ADAPTIVE_DTYPE).copy()
        return RegisteredPairs(results, mask_d.cpu().numpy(), idx, results["trials"].astype(np.int32), results["status"].astype(np.int32))

    def checked(self, ff, pc, dist_channels=5):
        """Synchronising status check of an extract() result: raises what the reference would raise."""
        raise_status(int(ff.status[0].item()))
        return ff

    def match_pose(self, fa, fb, rand):
        """Relative pose between two FrameFeatures (frame0 = fa, frame1 = fb), Match.py:241-283."""
        cur = torch.cuda.current_stream(self.device)
        for f in (fa, fb):          # rows produced on another lane: keep the allocator from recycling them early
            f.rows.record_stream(cur)
            f.n_key.record_stream(cur)
        idx = self.match(fa.features, fb.features, fa.n_key, fb.n_key)
        res, mask = self.ransac(fa.key_pts, fb.key_pts, idx, rand, fb.n_key)
        return res, mask, idx


    def match_pose_exact(self, fa, fb, rand, rand_host=None):
        """match_pose + the host half: -> (result record (_ffi.POSE_DTYPE), mask [1024] u8 (host), pair_idx (device)).  Synchronises."""
        cur = torch.cuda.current_stream(self.device)
        for f in (fa, fb):
            f.rows.record_stream(cur)
            f.n_key.record_stream(cur)
        idx = self.match(fa.features, fb.features, fa.n_key, fb.n_key)
        cert = self.new_cert(1)
        self.ransac(fa.key_pts, fb.key_pts, idx, rand, fb.n_key, cert=cert[0])
        results, masks, _, status = self.certify(cert, [rand_host if rand_host is not None else rand])
        if status[0] != 0:
            raise _ffi.CaeloError("pair could not be certified (status %d)" % status[0])
        return results[0], masks[0], idx


RegisteredPairs = collections.namedtuple("RegisteredPairs", "results masks pair_idx evals status")   # Engine.register_pairs

_default = None


def default_engine():
    global _default
    if _default is None:
        _default = Engine()
    return _default


_draws_tls = threading.local()


def ransac_draws(seed_or_rng, n=6000):
    """The uniform doubles RANSAC4RT would pull from NumPy's Mersenne Twister (Match.py:182).  An integer seed re-seeds a
    per-thread generator (the same stream as ``RandomState(seed)``): constructing a RandomState costs 116 us under the GIL -- four
    times the 6 000 draws, and what bounded run_sequence.py's loader threads."""
    if hasattr(seed_or_rng, "random_sample"):
        return seed_or_rng.random_sample(n)
    rs = getattr(_draws_tls, "rs", None)
    if rs is None:
        rs = _draws_tls.rs = np.random.RandomState(0)
    rs.seed(seed_or_rng)
    return rs.random_sample(n)
