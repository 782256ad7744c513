"""Odometry evaluation: the reference's three evaluation scripts restated.

    EvaluationOnRegistration.py / EvalOnReg_KeyPts.py   per-pair rotation / translation errors against ground truth
                                                        (Visualization.GetErrorRTs) -> the 7-column row of EvaluationResults.mat
    EvaluationOnKeypts.py                               key point repeatability: world-frame key points, nearest-neighbour distance
                                                        from frame i+1 to frame i (mode 0) or of a frame to itself (mode 1), and
                                                        histogram counts over Discretizations

The nearest-neighbour search runs on the device (caelo_kp_nn_pairs, csrc/evaluate.hip: scikit-learn's kd-tree distances, bit for
bit).  Everything else is O(frames) host arithmetic written with the reference's NumPy dtypes, casts and order, so that it gives
the reference's bits under the same NumPy (BLAS-dependent values may move by an ulp or two under another BLAS).

Deviations, both refused with ValueError: a fit set of 3 points or fewer (scikit-learn brute-forces those with a dot-product formula)
and a non-finite coordinate (scikit-learn raises there as well); a pose file whose row count is not the number of key point files.

Matchability (the inputs of the registration scripts, ``Matchablity_*.mat``): ``proportion = n_inliers / n_pairs`` as Match.py:217
prints it and ``trials = iterations`` (cntIters of RANSAC4RT's last level).  The published column 7 (100.8 trials) came from MATLAB's
3-point RANSAC (Scripts/GenerateTrajactory.m:213-221), not from RANSAC4RT: trial counts of this engine are not comparable with it.
"""
import os

import numpy as np
from numpy import linalg as LA
from scipy import io

from . import keysources, stageio
from .refine import GetLidarRelRtBetween2Poses, GetRtFromOnePose, RotateMat2EulerAngle_XYZ

DISCRETIZATIONS = [0.1, 0.2, 0.4, 0.8, 1.6, 3.2, 6.4]   # EvaluationOnKeypts.py:105 (metres)
T_RRE, T_RTE = 1.0, 0.5   # EvaluationOnRegistration.py:23-24 (degrees, metres)
SOURCES = ("ae", "3dfeatnet", "usip")   # iDataSource 0 / 1 / 2


# ---- key point repeatability (EvaluationOnKeypts.py) ----------------------------------------------------------------------------
def TranslatePtsIntoWorldFrame(pose, Tr, Pts):
    """Transformations.py:20-24: LiDAR points [K,3] -> world frame through Tr [3,4] then pose [3,4].  float32 for float32 points,
    float64 for float64 points (USIP, rotated by the float64 R90)."""
    ones = np.ones([Pts.shape[0], 1], dtype=np.float32)
    cam = np.dot(Tr, np.c_[Pts, ones].T)
    return np.dot(pose, np.r_[cam, ones.T]).T


def _frame_keypts(keypts_dir, source, frame):
    """One frame's key points as the reference reads them (EvaluationOnKeypts.py:43-57); no limit on K."""
    if source == "ae":
        return io.loadmat(keysources.features_dir_path(keypts_dir, frame))["KeyPts"]
    path = keysources.keypts_path(keypts_dir, frame)
    if source == "3dfeatnet":
        return keysources._fromfile(path, 3 + keysources.FEATURE_DIMENSION_1)[:, 0:3]
    if source == "usip":
        return np.dot(keysources.R90, keysources._fromfile(path, 3).T).T
    raise ValueError("key point source %r: one of %s" % (source, ", ".join(SOURCES)))


def GetAllKeyPts(keypts_dir, source, poses, Tr, iFrameStep=1):
    """EvaluationOnKeypts.py:18-65 with explicit paths: every iFrameStep-th frame's key points in the world frame.

    keypts_dir: ``<frame:06d>.bin.mat`` files (KeyPts field: the KeyPts/ or Features/ folders) for source 'ae', ``<frame:06d>.bin``
    for '3dfeatnet' ([-1, 35] f32) and 'usip' ([-1, 3] f32, rotated by R90).  The frame count is the number of files in the
    directory (:35-36).  poses: ground truth [n, 12]; Tr [3, 4] (any dtype: cast to float32 as at :28)."""
    if source not in SOURCES:
        raise ValueError("key point source %r: one of %s" % (source, ", ".join(SOURCES)))
    poses = np.asarray(poses).reshape(-1, 12)
    Tr = np.array(np.asarray(Tr).reshape(3, 4), dtype=np.float32)
    n = len(os.listdir(keypts_dir))
    if poses.shape[0] != n:
        raise ValueError("%d poses for %d key point files in %s: one pose per frame" % (poses.shape[0], n, keypts_dir))
    out = []
    for i in range(0, n, iFrameStep):
        pose = np.array(poses[i].reshape(3, 4), dtype=np.float32)
        out.append(TranslatePtsIntoWorldFrame(pose, Tr, _frame_keypts(keypts_dir, source, i)))
    return out


def stack_keypts(KeyPtsList):
    """A list of [K_i, 3] world-frame sets -> (pts [F, ld, 3] f64, n_key [F] i32), ld = max K_i (the layout of caelo_kp_nn_pairs)."""
    F = len(KeyPtsList)
    nk = np.array([a.shape[0] for a in KeyPtsList], dtype=np.int32)
    ld = max(1, int(nk.max()) if F else 1)
    pts = np.zeros((F, ld, 3), dtype=np.float64)
    for i, a in enumerate(KeyPtsList):
        pts[i, :a.shape[0]] = a
    return pts, nk


def _engine(engine):
    if engine is not None:
        return engine
    from .engine import Engine
    return Engine(respond_h5=None, encoder_h5=None)


def pair_list(n_frames, inner=False):
    """(fit, query) pairs of the stepped list: (k, k+1) for GetPairDistances, (k, k) for ComputeDispersionOfKeypoints."""
    k = np.arange(n_frames if inner else max(n_frames - 1, 0), dtype=np.int32)
    return np.stack([k, k if inner else k + 1], axis=1)


def check_sets(KeyPtsList, pairs, thresholds=DISCRETIZATIONS):
    """What the device pass refuses, checked on the host before any launch (ValueError): a fit set of 3 points or fewer
    (scikit-learn's NearestNeighbors takes its brute-force path there, _base.py:485-488, with another rounding), an empty query set,
    a non-finite coordinate (scikit-learn raises too), a set above the kernel's limit, thresholds that are not finite and positive."""
    from . import _ffi
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= thr.size <= _ffi.KP_NN_MAX_THRESHOLDS or not (np.isfinite(thr).all() and (thr > 0).all()):
        raise ValueError("thresholds: 1 to %d finite positive values, got %s" % (_ffi.KP_NN_MAX_THRESHOLDS, thr.tolist()))
    for i, a in enumerate(KeyPtsList):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("frame %d: key points must be [K, 3], got %s" % (i, a.shape))
        if a.shape[0] > _ffi.KP_NN_MAX_K:
            raise ValueError("frame %d holds %d key points: at most %d per set" % (i, a.shape[0], _ffi.KP_NN_MAX_K))
        if not np.isfinite(a).all():
            raise ValueError("frame %d: Input contains NaN, infinity or a value too large for dtype('float64')." % i)
    for f0, f1 in np.asarray(pairs).reshape(-1, 2):
        if KeyPtsList[f0].shape[0] <= 3:
            raise ValueError("frame %d holds %d key points: a fit set of 3 or fewer is brute-forced by scikit-learn (a different rounding), "
                             "which the device pass does not restate" % (f0, KeyPtsList[f0].shape[0]))
        if KeyPtsList[f1].shape[0] < 1:
            raise ValueError("frame %d holds no key points" % f1)


def device_distances(KeyPtsList, inner=False, thresholds=DISCRETIZATIONS, engine=None):
    """The device pass over a stepped key point list -> (distances [sum of query K, 1] f64 in the reference's order, counts [T+1]
    i64 summed over the pairs)."""
    pairs = pair_list(len(KeyPtsList), inner)
    check_sets(KeyPtsList, pairs, thresholds)
    eng = _engine(engine)
    pts, nk = stack_keypts(KeyPtsList)
    dist, counts = eng.kp_nn_pairs(pts, nk, pairs, thresholds)
    dist = dist.cpu().numpy()
    rows = [dist[p, :nk[q]] for p, q in enumerate(pairs[:, 1])]
    d = np.concatenate(rows).reshape(-1, 1) if rows else np.zeros((0, 1), np.float64)
    return d, counts.sum(dim=0).cpu().numpy()


def GetPairDistances(KeyPtsList, engine=None):
    """EvaluationOnKeypts.py:68-81 on the device: distance from every key point of frame k+1 to the nearest of frame k, [N, 1] f64."""
    return device_distances(KeyPtsList, False, engine=engine)[0]


def ComputeDispersionOfKeypoints(KeyPtsList, engine=None):
    """EvaluationOnKeypts.py:83-94 on the device.  The reference queries each frame's fit set with the same set, so every distance is
    0 (its own comment at :93 notes it); that is what is reproduced here, not a distance to the nearest OTHER point."""
    return device_distances(KeyPtsList, True, engine=engine)[0]


def RepeatabilityCounts(distances, Discretizations=DISCRETIZATIONS):
    """EvaluationOnKeypts.py:128-140 on the host: C_t = #(distances / D_t < 1), counts[t] = C_t - C_{t-1}, then #(distances / D_last
    >= 1).  -> list of NumPy ints (what the reference hands to savemat)."""
    counts, prev, scaled = [], 0, None
    for D in Discretizations:
        scaled = distances / D
        c = np.sum(scaled < 1)
        counts.append(c - prev)
        prev = c
    counts.append(np.sum(scaled >= 1))
    return counts


def repeatability(keypts_dir, source, poses, Tr, iFrameStep=1, inner=False, Discretizations=DISCRETIZATIONS, engine=None):
    """One sequence: GetAllKeyPts, the device pass (mode 0: pairs (k, k+1); inner / mode 1: (k, k)) -> (counts list of NumPy ints,
    distances [N, 1] f64)."""
    pts = GetAllKeyPts(keypts_dir, source, poses, Tr, iFrameStep)
    d, c = device_distances(pts, inner, Discretizations, engine)
    return [np.int64(v) for v in c], d


def repeatability_name(iFrameStep, source, seq, inner=False):
    """The reference's file name (EvaluationOnKeypts.py:98-101, :142): AccuracyOfKeyPts_<step>_<source>_<seq>.mat."""
    return "%s%d_%d_%s.mat" % ("InnerAccuracyOfKeyPts_" if inner else "AccuracyOfKeyPts_", iFrameStep, SOURCES.index(source), seq)


def save_repeatability(path, counts):
    """{'counts': counts} as the reference writes it (savemat of a Python list of NumPy ints: [1, T+1])."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    io.savemat(path, {"counts": [np.int64(c) for c in counts]})
    return path


# ---- registration errors (Visualization.py:152-172, EvaluationOnRegistration.py) ------------------------------------------------
def GetLidarRelRsAndTs(poses, Tr):
    """Transformations.py:127-139: consecutive relative motions in the LiDAR frame, [n-1, 3, 3] and [n-1, 3] f64."""
    R_Tr, T_Tr = GetRtFromOnePose(Tr)
    R_Tr_inv = np.linalg.inv(R_Tr)
    T_Tr_inv = -np.dot(R_Tr_inv, T_Tr)
    n = poses.shape[0] - 1
    Rs = np.zeros((n, 3, 3), dtype=np.float64)
    Ts = np.zeros((n, 3), dtype=np.float64)
    for i in range(n):
        R, T = GetLidarRelRtBetween2Poses(poses[i, :], poses[i + 1, :], R_Tr, T_Tr, R_Tr_inv, T_Tr_inv)
        Rs[i, :, :] = R
        Ts[i, :] = T.reshape(1, 3)
    return Rs, Ts


def _eulers(Rs):
    E = np.zeros((Rs.shape[0], 3), dtype=np.float64)
    for i in range(Rs.shape[0]):
        E[i, :] = RotateMat2EulerAngle_XYZ(Rs[i, :, :])
    return E


def GetLidarDiffRels(poses, Tr):
    """Transformations.py:141-150 -> [relRs, relTs, relEulers, diffNormRelEulers, diffNormRelTs]."""
    Rs, Ts = GetLidarRelRsAndTs(poses, Tr)
    E = _eulers(Rs)
    return [Rs, Ts, E, LA.norm(E[1:E.shape[0], :] - E[0:E.shape[0] - 1, :], axis=1), LA.norm(Ts[1:Ts.shape[0], :] - Ts[0:Ts.shape[0] - 1, :], axis=1)]


def GetErrorEulers(relRs0, relRs1):
    """Visualization.py:152-160: Euler angles (degrees) of inv(R0) R1 per pair, float32 [n, 3]."""
    if relRs0.shape[0] != relRs1.shape[0]:
        raise ValueError("%d and %d relative rotations" % (relRs0.shape[0], relRs1.shape[0]))
    out = np.zeros((relRs0.shape[0], 3), dtype=np.float32)
    for i in range(relRs0.shape[0]):
        out[i, :] = RotateMat2EulerAngle_XYZ(np.dot(np.linalg.inv(relRs0[i, :, :]), relRs1[i, :, :]))
    return out


def GetErrorRTs(poses, poses_, Tr, iFrameStep=1):
    """Visualization.py:163-241 without the plots: ground truth ``poses`` and estimate ``poses_`` [n, 12] (sliced [0:n:step] as at
    EvalOnReg_KeyPts.py:96-99, n = the ground truth's row count), Tr [3, 4] f32 -> (GroundTruthRels, EstimatedRels, errorRelEulers
    [m, 3] f32, errorRelTs [m, 3] f64)."""
    poses = np.asarray(poses).reshape(-1, 12)
    poses_ = np.asarray(poses_).reshape(-1, 12)
    n = poses.shape[0]
    poses, poses_ = poses[0:n:iFrameStep, :], poses_[0:n:iFrameStep, :]
    if poses.shape[0] != poses_.shape[0]:
        raise ValueError("%d ground truth poses and %d estimated poses" % (poses.shape[0], poses_.shape[0]))
    gt = GetLidarDiffRels(poses, Tr)
    est = GetLidarDiffRels(poses_, Tr)
    return gt, est, GetErrorEulers(gt[0], est[0]), est[1] - gt[1]


def read_tr(calib_path):
    """calib_.txt row 4 as float32 [3, 4] (EvaluationOnRegistration.py:61-63)."""
    return stageio.read_calib_tr(calib_path)


def RegistrationRow(sequences, t_RRE=T_RRE, t_RTE=T_RTE):
    """EvaluationOnRegistration.py:50-130 over one or more sequences (concatenated like its loop).  sequences: a list of
    (errorRelEulers, errorRelTs, AllProportions, AllTrialCounts), the last two as stored in a matchability file ([1, n]).
    -> float32 [7] = RRE, stdRRE, RTE, stdRTE, success rate (fraction), inlier ratio (fraction), average trials, and the success
    flags [m] bool."""
    E = np.zeros((1, 3), dtype=np.float32)
    T = np.zeros((1, 3), dtype=np.float32)
    P = np.zeros((1, 1), dtype=np.float32)
    N = np.zeros((1, 1), dtype=np.float32)
    for eul, t, prop, trials in sequences:
        E = np.r_[E, eul]
        T = np.r_[T, t]
        P = np.r_[P, np.asarray(prop).T]
        N = np.r_[N, np.asarray(trials).T]
    E, T, P, N = (np.delete(a, 0, axis=0) for a in (E, T, P, N))
    # :102-105: each through a one-element list, float32, squeezed
    E, T, P, N = (np.squeeze(np.array([a], dtype=np.float32)) for a in (E, T, P, N))
    RREs = np.sum(np.abs(E), axis=1)
    RTEs = LA.norm(T, axis=1)
    ok = (RREs < t_RRE) * (RTEs < t_RTE)
    row = np.zeros((7,), dtype=np.float32)
    row[:] = [np.mean(RREs), np.std(RREs), np.mean(RTEs), np.std(RTEs), np.sum(ok) / RREs.shape[0], np.mean(P), np.mean(N)]
    return row, ok


def matchability_arrays(n_inliers, n_pairs, iterations):
    """Per-pair RANSAC records -> (AllProportions, AllTrialCounts) [1, n] f64: n_inliers / n_pairs (Match.py:217) and cntIters."""
    n_inliers = np.asarray(n_inliers, dtype=np.float64).reshape(-1)
    n_pairs = np.asarray(n_pairs, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(n_pairs > 0, n_inliers / n_pairs, 0.0)
    return prop.reshape(1, -1), np.asarray(iterations, dtype=np.float64).reshape(1, -1)


def save_matchability(path, n_inliers, n_pairs, iterations):
    """``Matchablity_*.mat``: AllProportions / AllTrialCounts [1, n] f64 (the registration scripts read ``mat[...].T``)."""
    prop, trials = matchability_arrays(n_inliers, n_pairs, iterations)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    io.savemat(path, {"AllProportions": prop, "AllTrialCounts": trials})
    return path


def load_matchability(path):
    m = io.loadmat(path)
    return m["AllProportions"], m["AllTrialCounts"]


def registration(gt_paths, est_paths, calib_paths, matchability_paths, iFrameStep=1):
    """The registration row over sequences given as files (one of each per sequence) -> (row [7] f32, success flags)."""
    if not (len(gt_paths) == len(est_paths) == len(calib_paths) == len(matchability_paths)):
        raise ValueError("one --gt, --est, --calib and --matchability per sequence")
    seqs = []
    for g, e, c, m in zip(gt_paths, est_paths, calib_paths, matchability_paths):
        _, _, eul, t = GetErrorRTs(np.loadtxt(g), np.loadtxt(e), read_tr(c), iFrameStep)
        prop, trials = load_matchability(m)
        seqs.append((eul, t, prop, trials))
    return RegistrationRow(seqs)


def save_registration(path, row):
    """EvaluationResults [1, 7] f32 (EvaluationOnRegistration.py:133)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    io.savemat(path, {"EvaluationResults": np.asarray(row, dtype=np.float32).reshape(1, 7)})
    return path



# ---- loop closures (detect_loops.py's loops file against ground truth) -----------------------------------------------------------
def lidar_positions(poses, Tr):
    """Ground truth poses [n, 12] (camera frame) and Tr [3, 4] -> the LiDAR's world positions [n, 3] f64: pose applied to Tr's origin."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3, 4)
    t_tr = np.asarray(Tr, dtype=np.float64).reshape(3, 4)[:, 3]
    return poses[:, :, 0:3] @ t_tr + poses[:, :, 3]


def revisits(positions, revisit_radius=4.0, min_gap=50):
    """-> [n, n] bool: frame j <= i - min_gap lies within revisit_radius metres of frame i (all pairs on the host)."""
    p = np.asarray(positions, dtype=np.float64)
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))
    i, j = np.mgrid[0:len(p), 0:len(p)]
    return (d < revisit_radius) & (j <= i - min_gap)


def loops(poses, Tr, loop_rows, revisit_radius=4.0, min_gap=50):
    """Detected loops [m, 19] (caelo.loops: i j dist shift verified n_inliers threshold R(9) T(3)) against ground truth poses.
    -> dict: n_revisit_queries (frames with a ground-truth revisit), recall (those for which a detected loop is a true revisit),
    precision / precision_verified (detected / verified loops that are true revisits; nan without any), and for the verified loops
    the errors of (R, T) against the ground-truth motion of frame i into frame j in the LiDAR frame: error_eulers [v, 3] degrees
    (GetErrorEulers), error_ts [v, 3] metres, RRE / RTE [v] as sums of absolute components, RTE_norm [v], and success [v] =
    RRE < 1 degree and RTE < 0.5 m (EvaluationOnRegistration.py:22-23)."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    rows = np.asarray(loop_rows, dtype=np.float64).reshape(-1, 19)
    n = poses.shape[0]
    li, lj = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    if rows.size and (li.min() < 0 or li.max() >= n or lj.min() < 0 or lj.max() >= n):
        raise ValueError("a loop names a frame outside the %d ground truth poses" % n)
    rev = revisits(lidar_positions(poses, Tr), revisit_radius, min_gap)
    true = rev[li, lj]
    has = rev.any(axis=1)
    found = np.zeros(n, dtype=bool)
    found[li[true]] = True
    ver = rows[:, 4] > 0
    R_Tr, T_Tr = GetRtFromOnePose(np.asarray(Tr, dtype=np.float64))
    R_Tr_inv = np.linalg.inv(R_Tr)
    T_Tr_inv = -np.dot(R_Tr_inv, T_Tr)
    gtR = np.zeros((int(ver.sum()), 3, 3))
    gtT = np.zeros((int(ver.sum()), 3))
    for k, r in enumerate(rows[ver]):
        R, T = GetLidarRelRtBetween2Poses(poses[int(r[1])], poses[int(r[0])], R_Tr, T_Tr, R_Tr_inv, T_Tr_inv)
        gtR[k], gtT[k] = R, T.reshape(3)
    eul = GetErrorEulers(gtR, rows[ver, 7:16].reshape(-1, 3, 3))
    err_t = rows[ver, 16:19] - gtT
    rre, rte = np.abs(eul).sum(axis=1).astype(np.float64), np.abs(err_t).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(n_revisit_queries=int(has.sum()), n_loops=len(rows), n_verified=int(ver.sum()),
                    recall=float(np.float64((found & has).sum()) / has.sum()), precision=float(np.float64(true.sum()) / len(rows)),
                    precision_verified=float(np.float64((true & ver).sum()) / ver.sum()), error_eulers=eul, error_ts=err_t, RRE=rre, RTE=rte,
                    RTE_norm=LA.norm(err_t, axis=1), success=(rre < T_RRE) & (rte < T_RTE))


# ---- reconstruction quality of an autoencoder (AE4VoxelPatch.py:213,228,242-284) ----------------------------------------------------
def reconstruction(engine, scans, threshold=0.1):
    """How well the engine's autoencoder (Engine.load_autoencoder) rebuilds the patches of ``scans`` (an iterable of [N,4] f32 clouds):
    per frame the key points, patches and descriptors of ``Engine.extract``, then ``Engine.decode`` of the resident descriptor rows
    against the patches.  -> dict: ``n_key`` [F] i32, ``loss`` [F,3] f32 the mean binary_crossentropy per frame and scale, ``iou``
    [F,3] f64 = both / (in + out - both) over a frame's patches of a scale (voxels set in the patch, in the reconstruction at
    ``threshold``, in both; NaN when neither has a voxel), ``patch_loss`` [sum K,3] f32 every patch's loss, ``mean_loss`` the mean over
    all patches in float64 -- Keras's validation-loss figure for them."""
    import torch
    from .engine import raise_status
    n_key, loss, iou, per_patch = [], [], [], []
    for pc in scans:
        pc = pc if isinstance(pc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32))
        ff = engine.extract(pc.to(engine.device).contiguous())
        bits = engine.extract_patch_bits()
        raise_status(int(ff.status[0].item()))
        k = int(ff.n_key.item())
        if k < 1:   # (the detector's own check, raise_status, refuses fewer than 51 key points: this guards other sources of rows)
            raise ValueError("frame %d has no key points: nothing to reconstruct" % len(n_key))
        d = engine.decode(ff.rows[:k].contiguous(), group=3, target=bits[:k].contiguous(), threshold=threshold, bits=False)
        l = d.loss.view(k, 3).cpu().numpy()
        c = d.counts.view(k, 3, 3).cpu().numpy().astype(np.int64).sum(axis=0)   # [scale][in, out, both]
        union = c[:, 0] + c[:, 1] - c[:, 2]
        n_key.append(k)
        per_patch.append(l)
        loss.append(l.mean(axis=0, dtype=np.float64).astype(np.float32))
        iou.append(np.where(union > 0, c[:, 2] / np.maximum(union, 1), np.nan))
    if not n_key:
        raise ValueError("no scans to evaluate")
    per_patch = np.concatenate(per_patch)
    return dict(n_key=np.asarray(n_key, np.int32), loss=np.stack(loss), iou=np.stack(iou), patch_loss=per_patch,
                mean_loss=float(per_patch.mean(dtype=np.float64)), threshold=float(threshold))


def save_reconstruction(path, res):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    io.savemat(path, {"n_key": res["n_key"], "loss": res["loss"], "iou": res["iou"], "patch_loss": res["patch_loss"],
                      "mean_loss": np.float64(res["mean_loss"]), "threshold": np.float64(res["threshold"])})
