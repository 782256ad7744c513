"""Key point sources other than the auto-encoder detector (PoseEstimation.py:26-45, :132-143, :176-177).

The reference's pair loop runs on three key point sources (``iKeyPtSource``):

    0  its own detector (GetKeyPtsByAE)           -> Engine.extract / Pipeline.run as before
    1  3DFeatNet key points: <seq>/<frame:06d>.bin, [-1, 35] f32, xyz in columns 0:3 (FEATURE_DIMENSION_1 = 32 descriptor columns)
    2  USIP key points: <seq>/<frame:06d>.bin, [-1, 3] f32 (``tsf_1024``, Dirs.py:37), rotated by R90 (:39, :177)

and a features-from-file mode (``isLoadFeaturesFromFile``, :49-66) that reads KeyPts / Features / Weights from ``Features/*.mat`` and
runs only the pair stage.  This module reads those inputs; the fused path takes them through ``Engine.extract(key_pts=...)`` and
``Pipeline.run(keypts=..., rows_given=...)`` (include/caelo.h CAELO_EXTRACT_GIVEN_KEYPTS / CAELO_EXTRACT_GIVEN_ROWS).

USIP precision: the reference keeps the rotated points in float64 through GetPatchesList and RANSAC4RT; the engine carries key
points in float32 (like ``api._dev``), so ``read_usip`` rounds the float64 product to float32.  The rotation itself is NumPy's,
done exactly as the reference does it, so the float32 points are the reference's rounded once.

The fused path serves at most 1024 key points per frame (CAELO_MAX_KEYPTS); a larger set is refused with an error that names the
staged API, which has no such limit.
"""
import math
import os

import numpy as np

MAX_K = 1024
FEATURE_DIMENSION_1 = 32   # PoseEstimation.py:176 (3DFeatNet descriptor width)


def EulerAngle2RotateMat(angX, angY, angZ, RotateSequnce):
    """Transformations.py:188-212: R = R_s2 R_s1 R_s0 for the rotation sequence, float64."""
    R = np.eye(3, dtype=np.float64)
    R_X = np.array([[1, 0, 0], [0, math.cos(angX), -math.sin(angX)], [0, math.sin(angX), math.cos(angX)]], dtype=np.float64)
    R_Y = np.array([[math.cos(angY), 0, math.sin(angY)], [0, 1, 0], [-math.sin(angY), 0, math.cos(angY)]], dtype=np.float64)
    R_Z = np.array([[math.cos(angZ), -math.sin(angZ), 0], [math.sin(angZ), math.cos(angZ), 0], [0, 0, 1]], dtype=np.float64)
    for c in RotateSequnce[:3]:
        if c in "xX":
            R = np.dot(R_X, R)
        elif c in "yY":
            R = np.dot(R_Y, R)
        elif c in "zZ":
            R = np.dot(R_Z, R)
        else:
            raise ValueError("rotation sequence %r: axes are x, y, z" % (RotateSequnce,))
    return R


R90 = EulerAngle2RotateMat(-math.pi / 2, 0, -math.pi / 2, "xyz")   # PoseEstimation.py:177


def keypts_path(keypts_dir, frame):
    """<dir>/<frame:06d>.bin, the reference's naming (PoseEstimation.py:33,:37)."""
    return os.path.join(keypts_dir, str(int(frame)).zfill(6) + ".bin")


def check_count(k, what="key point set"):
    if k > MAX_K:
        raise ValueError("%s holds %d key points: the fused path (Engine.extract / Pipeline.run / run_sequence.py) serves at most %d "
                         "per frame -- use the staged API (caelo.api.Voxelization -> GetPatchesList -> GetFeaturesFromPatches -> "
                         "SolveRelativePose), which has no such limit" % (what, k, MAX_K))
    return k


def _fromfile(path, cols):
    if not os.path.isfile(path):
        raise FileNotFoundError("key point file %s does not exist (expected <keypts-dir>/<frame:06d>.bin)" % path)
    a = np.fromfile(path, dtype=np.float32, count=-1)
    if a.size % cols:
        raise ValueError("%s: %d floats do not make rows of %d" % (path, a.size, cols))
    return a.reshape([-1, cols])


def read_3dfeatnet(path, descriptors=False):
    """3DFeatNet .bin (PoseEstimation.py:33-35): [-1, 35] f32 -> key points [K,3] f32 (and the [K,32] descriptors)."""
    a = _fromfile(path, 3 + FEATURE_DIMENSION_1)
    check_count(a.shape[0], path)
    pts = np.ascontiguousarray(a[:, 0:3])
    return (pts, np.ascontiguousarray(a[:, 3:])) if descriptors else pts


def read_usip_f64(path):
    """USIP .bin (PoseEstimation.py:37-39): [-1, 3] f32 rotated by R90 with NumPy exactly as the reference does it -> [K,3] f64."""
    a = _fromfile(path, 3)
    check_count(a.shape[0], path)
    return np.dot(R90, a.T).T


def read_usip(path):
    """read_usip_f64 rounded to float32, the precision the engine carries key points in (see the module note)."""
    return np.ascontiguousarray(read_usip_f64(path), dtype=np.float32)


def write_3dfeatnet(path, pts, desc=None):
    """The 3DFeatNet file layout ([K, 35] f32; zero descriptors when none are given)."""
    pts = np.asarray(pts, dtype=np.float32)
    d = np.zeros((pts.shape[0], FEATURE_DIMENSION_1), np.float32) if desc is None else np.asarray(desc, dtype=np.float32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.ascontiguousarray(np.c_[pts, d], dtype=np.float32).tofile(path)
    return path


def write_usip(path, pts):
    """The USIP file layout ([K, 3] f32, in USIP's own axes: read_usip applies R90)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.ascontiguousarray(pts, dtype=np.float32).tofile(path)
    return path


SOURCES = {"3dfeatnet": read_3dfeatnet, "usip": read_usip}


def load_keypts(source, keypts_dir, frame):
    """Key points of ``frame`` from ``source`` ('3dfeatnet' | 'usip') as [K,3] f32."""
    if source not in SOURCES:
        raise ValueError("key point source %r: one of %s" % (source, ", ".join(sorted(SOURCES))))
    return SOURCES[source](keypts_path(keypts_dir, frame))


def rows_from_features(KeyPts, Features):
    """KeyPts [K,3] + Features [K,D<=60] -> the engine's rows [K,64] f32: descriptor zero-padded to columns 0:60 | xyz 60:63 | valid 63.
    Zero columns add nothing to a float64 Euclidean distance, so matching the rows is cdist(Features0, Features1)'s argmin."""
    KeyPts = np.asarray(KeyPts)
    Features = np.asarray(Features)
    k = check_count(KeyPts.shape[0], "features set")
    if Features.shape[0] != k or Features.ndim != 2 or Features.shape[1] > 60:
        raise ValueError("Features [K, D <= 60] for K = %d key points, got %s (descriptors wider than the rows' 60 columns go beside "
                         "the rows: Engine.register_pairs(..., desc=) / api.SolveRelativePoses(..., desc=))" % (k, Features.shape))
    rows = np.zeros((k, 64), np.float32)
    rows[:, 0:Features.shape[1]] = Features
    rows[:, 60:63] = KeyPts[:, 0:3]
    rows[:, 63] = 1.0
    return rows


def desc_path(desc_dir, frame):
    """<dir>/<frame:06d>.bin, the naming of the published comparison's descriptor folders (Scripts/GenerateTrajactory.m:193)."""
    return os.path.join(desc_dir, str(int(frame)).zfill(6) + ".bin")


def read_descriptors(path, dim):
    """A descriptor .bin of the published comparison (Scripts/GenerateTrajactory.m:193-197): [-1, dim] f32 -> [K, dim] f32."""
    dim = int(dim)
    if dim < 1:
        raise ValueError("%s: descriptor width %d, expected >= 1" % (path, dim))
    if not os.path.isfile(path):
        raise FileNotFoundError("descriptor file %s does not exist (expected <desc-dir>/<frame:06d>.bin)" % path)
    nbytes = os.path.getsize(path)
    if nbytes % (4 * dim):
        raise ValueError("%s: %d bytes do not make rows of %d float32 (%d bytes each)" % (path, nbytes, dim, 4 * dim))
    a = np.fromfile(path, dtype=np.float32, count=-1).reshape([-1, dim])
    check_count(a.shape[0], path)
    return a


def write_descriptors(path, desc):
    """The layout read_descriptors reads: the rows of ``desc`` [K, dim] as f32, nothing else."""
    desc = np.asarray(desc)
    if desc.ndim != 2 or desc.shape[1] < 1:
        raise ValueError("%s: descriptors [K, dim >= 1], got %s" % (path, desc.shape))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.ascontiguousarray(desc, dtype=np.float32).tofile(path)
    return path


class DescSource:
    """run_sequence.py --desc-dir: descriptors of another method (<desc_dir>/<frame:06d>.bin, [-1, desc_dim] f32) on key points that
    come from ``keypts_source`` ('3dfeatnet' | 'usip') + ``keypts_dir`` or from the KeyPts of ``features_from`` files (whose Features
    are ignored).  No scan is read.  Everything that is wrong with the arguments or with a frame's files is a ValueError that names
    the frame."""
    MAX_DIM = 256

    def __init__(self, desc_dir, desc_dim, keypts_source="ae", keypts_dir=None, features_from=None):
        if desc_dim is None:
            raise ValueError("--desc-dir needs --desc-dim, the descriptors' width: frame 0's file %s cannot be cut into rows without it" % desc_path(desc_dir, 0))
        if not 1 <= int(desc_dim) <= self.MAX_DIM:
            raise ValueError("--desc-dim %s: the match takes widths 1 .. %d (frame 0: %s)" % (desc_dim, self.MAX_DIM, desc_path(desc_dir, 0)))
        if keypts_source != "ae" and features_from:
            raise ValueError("--keypts-source and --features-from exclude each other (frame 0's key points: one source)")
        if keypts_source == "ae" and not features_from:
            raise ValueError("--desc-dir reads no scans: the key points of frame 0 and every other frame must come from --keypts-source "
                             "3dfeatnet|usip with --keypts-dir, or from the KeyPts of --features-from files")
        if keypts_source != "ae" and not keypts_dir:
            raise ValueError("--keypts-source %s needs --keypts-dir (frame 0: <keypts-dir>/000000.bin)" % keypts_source)
        self.desc_dir, self.dim = desc_dir, int(desc_dim)
        self.keypts_source, self.keypts_dir, self.features_from = keypts_source, keypts_dir, features_from

    def n_frames(self):
        """Frames 0 .. n - 1: the run of consecutive <frame:06d>.bin files from 000000.bin on."""
        n = 0
        while os.path.isfile(desc_path(self.desc_dir, n)):
            n += 1
        return n

    def frame(self, i):
        """-> (key points [K,3] f32, descriptors [K,dim] f32) of frame i."""
        if self.features_from:
            pts = np.ascontiguousarray(np.asarray(load_features_dir(self.features_from, i)[0])[:, 0:3], dtype=np.float32)
            check_count(pts.shape[0], "frame %d's features file" % i)
        else:
            pts = load_keypts(self.keypts_source, self.keypts_dir, i)
        try:
            d = read_descriptors(desc_path(self.desc_dir, i), self.dim)
        except ValueError as e:
            raise ValueError("frame %d: %s" % (i, e))
        if d.shape[0] != pts.shape[0]:
            raise ValueError("frame %d: %d key points but %d descriptors of width %d in %s" % (i, pts.shape[0], d.shape[0], self.dim,
                                                                                             desc_path(self.desc_dir, i)))
        return pts, d


def load_features(raw_file, folder="Features"):
    """``Features/<scan>.mat`` of a raw scan (PoseEstimation.py:54-61) -> (KeyPts, Features, Weights), through stageio."""
    from . import stageio
    path = stageio.mat_path(raw_file, folder)
    if not os.path.isfile(path):
        raise FileNotFoundError("features file %s does not exist" % path)
    return stageio.load_keypts_and_features(raw_file, folder)


def features_dir_path(features_dir, frame):
    """<dir>/<frame:06d>.bin.mat, the reference's naming of its features base directory (PoseEstimation.py:52-56)."""
    return os.path.join(features_dir, str(int(frame)).zfill(6) + ".bin.mat")


def load_features_dir(features_dir, frame):
    """(KeyPts, Features, Weights) of ``frame`` from a features directory (isLoadFeaturesFromFile, PoseEstimation.py:52-61)."""
    d = os.path.abspath(features_dir)
    raw = os.path.join(os.path.dirname(d), "velodyne", str(int(frame)).zfill(6) + ".bin")   # stageio.mat_path(raw, basename(d)) is the file
    return load_features(raw, os.path.basename(d))


def save_features(raw_file, KeyPts, Features, Weights=None, folder="Features"):
    """Writes what load_features reads (stageio.save_features, PoseEstimation.py:280-295)."""
    from . import stageio
    return stageio.save_features(raw_file, KeyPts, Features, Weights, folder)
