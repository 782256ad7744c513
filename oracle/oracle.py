"""Python face of the CPU oracle (TEST INFRASTRUCTURE ONLY -- see caelo_oracle.c header).

Mirrors the reference's function-level call surface on NumPy arrays so
parity tests read like calls into the reference:

    ProjectPC2SphericalRing   SphericalRing.py:72      GetPatchesList          Voxel.py:177
    GetKeyPtsByAE             SphericalRing.py:113     GetFeaturesFromPatches  Match.py:130
    Voxelization              Voxel.py:100             SolveRT / RANSAC4RT / SolveRelativePose
                                                        Match.py:138 / :162 / :241

Heavy loops live in caelo_oracle.c (ctypes); the 3x3 SVD and RANSAC control flow are NumPy
(LAPACK), exactly like the reference.  Only tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg may import this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_build", "liboracle.so")

IMG_H, IMG_W, RING_C = 69, 1800, 5
NET_H, NET_W = 64, 1792
VIS = np.array([99.84, 99.84, 14.72], dtype=np.float64)  # Voxel.py:50-52
VOXEL_SIZES = [0.02, 0.02 * 8, 0.02 * 32]               # Voxel.py:31


def build(force=False):
    if force or not os.path.exists(_LIB_PATH) or (
            os.path.getmtime(_LIB_PATH) < os.path.getmtime(os.path.join(_HERE, "caelo_oracle.c"))):
        subprocess.check_call(["make", "-C", _HERE, "-B" if force else "-s"],
                              stdout=subprocess.DEVNULL)
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_LIB_PATH)
        _lib.orc_num_threads.restype = C.c_int
        _lib.orc_argpartition_fallbacks.restype = C.c_int64
    return _lib


def _p(a, t=C.c_void_p):
    return a.ctypes.data_as(t)


def num_threads():
    return lib().orc_num_threads()


def set_num_threads(n):
    lib().orc_set_num_threads(int(n))


# ---------------------------------------------------------------------------------------------
def ProjectPC2SphericalRing(PC):
    """SphericalRing.py:72-94 -> (Image_float [69,1800,5] f32, GridCounter [69,1800] i32)."""
    assert PC.shape[0] > 3 and PC.shape[1] == 4  # :73
    PC = np.ascontiguousarray(PC, dtype=np.float32)
    ring = np.empty((IMG_H, IMG_W, RING_C), dtype=np.float32)
    cnt = np.empty((IMG_H, IMG_W), dtype=np.int32)
    rc = lib().orc_project(_p(PC), C.c_int64(PC.shape[0]), _p(ring), _p(cnt))
    if rc != 0:
        raise IndexError("index 1800 is out of bounds for axis 1 with size 1800")
    return ring, cnt


class RespondLayer:
    """Stand-in for keras ``load_model(SphericalRingPCRespondLayer.h5)``; ``predict`` follows
    the h5 model_config (Conv2D 3->32 3x3 same relu, Conv2D 32->8 1x1 relu)."""

    def __init__(self, w1, b1, w2, b2):
        self.w1 = np.ascontiguousarray(w1, np.float32).reshape(3, 3, 3, 32)
        self.b1 = np.ascontiguousarray(b1, np.float32)
        self.w2 = np.ascontiguousarray(w2, np.float32).reshape(32, 8)
        self.b2 = np.ascontiguousarray(b2, np.float32)

    def predict(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 4 and x.shape[1:] == (NET_H, NET_W, 3)
        out = np.empty((x.shape[0], NET_H, NET_W, 8), dtype=np.float32)
        for b in range(x.shape[0]):
            lib().orc_respond(_p(x[b]), C.c_int(NET_W), C.c_int(3), _p(self.w1), _p(self.b1),
                              _p(self.w2), _p(self.b2), _p(out[b]))
        return out


def GetKeyPtsByAE(SphericalRing, GridCounter, RespondImg, return_score=False):
    """SphericalRing.py:113-291.  Demo mode: full [69,1800,5] ring; batch mode: cropped
    [64,1792,3] ring (BatchPreprocess.py:97-98,131-136)."""
    ring = np.ascontiguousarray(SphericalRing, dtype=np.float32)
    cnt = np.ascontiguousarray(GridCounter, dtype=np.int32)
    resp = np.ascontiguousarray(RespondImg, dtype=np.float32)
    assert resp.shape == (NET_H, NET_W, 8)
    kpix = np.zeros((1024, 2), dtype=np.int64)
    kpts = np.zeros((1024, 3), dtype=np.float32)
    score = np.zeros((NET_H, NET_W), dtype=np.float32) if return_score else None
    k = lib().orc_keypoints(_p(ring), C.c_int(ring.shape[1]), C.c_int(ring.shape[2]), _p(cnt),
                            C.c_int(cnt.shape[1]), _p(resp), _p(kpix), _p(kpts),
                            _p(score) if return_score else None)
    assert k > 50  # :286
    out = (kpts[:k].copy(), kpix[:k].copy(), np.array([], dtype=np.float32))
    return out + (score,) if return_score else out


def ExtendKeyPtsInShpericalRing(SphericalRing, GridCounter, KeyPixels):
    """SphericalRing.py:294-317, statement by statement (NumPy; K <= 1024 windows).  MUTATES GridCounter like the
    reference (:307)."""
    r = 6                                                                # nNeighborRadius (:295)
    out = [np.zeros((0, 3), np.float32)]
    for iX, iY in np.asarray(KeyPixels).reshape(-1, 2):                  # :300-302
        mask = GridCounter[iX - r:iX + r + 1, iY - r:iY + r + 1]         # :304 (a view)
        nb = SphericalRing[iX - r:iX + r + 1, iY - r:iY + r + 1, 0:3]    # :305
        out.append(np.asarray(nb[mask > 0], np.float32))                 # :306, row-major over the window
        mask[:] = 0                                                      # :307
    return np.concatenate(out, axis=0)                                   # :314-316


def RotateMat2EulerAngle_XYZ(R):
    """Transformations.py:181-186 (degrees)."""
    import math
    return np.array([math.atan2(R[2, 1], R[2, 2]), math.atan2(-R[2, 0], math.sqrt(R[2, 1] ** 2 + R[2, 2] ** 2)),
                     math.atan2(R[1, 0], R[0, 0])]) * (180.0 / math.pi)


def nearest_neighbours(PC0, PC1, chunk=256):
    """sklearn NearestNeighbors(n_neighbors=1).fit(PC0).kneighbors(PC1) restated as a brute-force float64 search
    (exact Euclidean distance, first minimum) -> (distances [n1], indices [n1])."""
    a = np.asarray(PC0, np.float64)
    b = np.asarray(PC1, np.float64)
    dist = np.empty(len(b)); idx = np.empty(len(b), np.int64)
    for s in range(0, len(b), chunk):
        d = b[s:s + chunk, None, :] - a[None, :, :]
        d2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
        idx[s:s + chunk] = d2.argmin(axis=1)
        dist[s:s + chunk] = np.sqrt(d2.min(axis=1))
    return dist, idx


def _gate_margin(distances, threshold):
    """Smallest |distance - threshold| of one gate (inf for no distances): how far the gate is from flipping a pair."""
    d = np.asarray(distances, np.float64)
    return float(np.abs(d - threshold).min()) if d.size else float("inf")


def _icp_step(steps, iterations, success, n_pts, n_planar, thr0, thr1, R_star, T_star, margin, moved):
    """One entry of ``steps``: the loop's state after an iteration, as caelo_icp reports it when max_iter ends there --
    iterations that moved the clouds so far, isSuccess, the pair counts of this iteration, the thresholds AFTER this
    iteration's decay, R_star / T_star, the smallest gate margin of this iteration and whether the clouds moved."""
    if steps is not None:
        steps.append(dict(iterations=int(iterations), success=bool(success), n_pts=int(n_pts), n_planar=int(n_planar),
                          thr0=float(thr0), thr1=float(thr1), R_star=np.array(R_star, np.float64),
                          T_star=np.array(T_star, np.float64).reshape(3), margin=float(margin), moved=bool(moved)))


def ICP(PC0, PC1, maxIterTimes=50, minIterTimes=20 - 1, inlierThreshold=0.5, smallShiftThreshold=0.05, decay_rate=0.9, ep=0.001,
        trace=None, steps=None):
    """MyICP.py:26-72, statement by statement.  ``trace``: (pairs, threshold used) per fitted iteration; ``steps``: one
    _icp_step record per evaluated iteration, the one that finds too few pairs included."""
    PC0 = np.asarray(PC0); PC1 = np.asarray(PC1)
    R_star = np.eye(3, dtype=np.float64)
    T_star = np.zeros((3, 1), dtype=np.float64)
    for iIter in range(maxIterTimes):
        distances, indices = nearest_neighbours(PC0, PC1)                # :31-32
        idx1 = distances < inlierThreshold                               # :35
        idx0 = indices[idx1]                                             # :36-37
        margin = _gate_margin(distances, inlierThreshold)
        if idx0.shape[0] < 100:                                          # :38-40
            _icp_step(steps, iIter, False, idx0.shape[0], 0, inlierThreshold, 0.0, R_star, T_star, margin, False)
            return R_star, T_star, False
        R, T, _ = SolveRT(PC0[idx0, :], PC1[idx1, :])                    # :42-46
        PC1 = (np.dot(R, PC1.T) + T).T                                   # :49
        R_star = np.dot(R, R_star)                                       # :50
        T_star = np.dot(R, T_star) + T                                   # :51
        normEulers = np.linalg.norm(RotateMat2EulerAngle_XYZ(R))         # :54-55
        normT = np.linalg.norm(T)                                        # :56
        if trace is not None:
            trace.append((int(idx0.shape[0]), float(inlierThreshold)))
        converged = iIter >= minIterTimes and normEulers < ep and normT < ep   # :57-59
        if not converged and normEulers < smallShiftThreshold and normT < smallShiftThreshold:   # :63-65
            inlierThreshold *= decay_rate
        _icp_step(steps, iIter + 1, True, idx0.shape[0], 0, inlierThreshold, 0.0, R_star, T_star, margin, True)
        if converged:
            break
    return R_star, T_star, True


def GetPtsInliners(PC0, PC1, inlierThreshold, margins=None):
    """MyICP.py:75-85.  ``margins``: list that receives this gate's margin."""
    distances, indices = nearest_neighbours(PC0, PC1)
    idx1 = distances < inlierThreshold
    if margins is not None:
        margins.append(_gate_margin(distances, inlierThreshold))
    return PC0[indices[idx1], :], PC1[idx1, :]


def GetPlanarPtsInliners(PtsWithNorm0, PtsWithNorm1, inlierThreshold0, inlierThreshold1, margins=None):
    """MyICP.py:88-114: planar pairs = (foot of the perpendicular from the frame-0 neighbour onto the plane through the
    frame-1 point, that point).  An empty set raises like sklearn's fit (:94).  ``margins``: list that receives the
    margins of both gates."""
    PC0, PC1, Norms1 = PtsWithNorm0[:, 0:3], PtsWithNorm1[:, 0:3], PtsWithNorm1[:, 3:6]
    if PC0.shape[0] == 0 or PC0.ndim != 2 or PC0.shape[1] == 0:
        raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (PC0.shape,))
    distances, indices = nearest_neighbours(PC0, PC1)                    # :94-95
    idx1 = distances < inlierThreshold1                                  # :98
    inliers0, inliers1, norms1 = PC0[indices[idx1], :], PC1[idx1, :], Norms1[idx1, :]
    vetors = inliers0 - inliers1                                         # :104
    dist2Planes = np.sum(norms1 * vetors, axis=1)                        # :105
    pedals = inliers1 + norms1 * np.tile(dist2Planes.reshape(dist2Planes.shape[0], 1), [1, 3])   # :106
    d = np.linalg.norm(pedals - inliers1, axis=1)                        # :108
    idx = (d < inlierThreshold0).flatten()                               # :109
    if margins is not None:
        margins += [_gate_margin(distances, inlierThreshold1), _gate_margin(d, inlierThreshold0)]
    return pedals[idx, :], inliers1[idx, :]


def ICP_Pt2PtAndPt2Plane(PC0, PC1, PtsWithNorm0, PtsWithNorm1, maxIterTimes=50, minIterTimes=20 - 1, inlierThreshold0=0.5,
                         decay_rate0=0.9, inlierThreshold1=2.0, decay_rate1=0.5, smallShiftThreshold=0.1, ep=0.01, rng=None, trace=None,
                         steps=None):
    """MyICP.py:127-201, statement by statement (rng: RandomState standing in for NumPy's global generator at :137).
    ``trace``: (point pairs, planar pairs, thresholds used) per fitted iteration; ``steps``: one _icp_step record per
    evaluated iteration, the one that finds too few pairs included."""
    PC0 = np.asarray(PC0); PC1 = np.asarray(PC1)
    PtsWithNorm0 = np.asarray(PtsWithNorm0); PtsWithNorm1 = np.array(PtsWithNorm1)
    R_star = np.eye(3, dtype=np.float64)
    T_star = np.zeros((3, 1), dtype=np.float64)
    nMaxPts = 2000                                                       # :135
    if PtsWithNorm1.shape[0] > nMaxPts:
        RandIdxes = (rng or np.random).random_sample((nMaxPts,)) * PtsWithNorm1.shape[0]
        PtsWithNorm1 = PtsWithNorm1[np.array(RandIdxes, dtype=np.int32), :]
    isSuccess = True
    for iIter in range(maxIterTimes):
        margins = []
        in0p, in1p = GetPtsInliners(PC0, PC1, inlierThreshold0, margins)   # :145
        if iIter < 100:                                                  # :147-150
            in0q, in1q = GetPlanarPtsInliners(PtsWithNorm0, PtsWithNorm1, inlierThreshold0, inlierThreshold1, margins)
            inliers0, inliers1 = np.r_[in0p, in0q], np.r_[in1p, in1q]
        else:                                                            # :151-153: the planar pairs of iteration 99, both
            inliers0, inliers1 = in0q, in1q                              # arrays as they were then -- the same (R, T) every time
        if inliers0.shape[0] < 200:                                      # :166-169
            if iIter < 1:
                isSuccess = False
            _icp_step(steps, iIter, isSuccess, in0p.shape[0], in0q.shape[0], inlierThreshold0, inlierThreshold1, R_star, T_star,
                      min(margins), False)
            break
        R, T, _ = SolveRT(inliers0, inliers1)                            # :172
        PC1 = (np.dot(R, PC1.T) + T).T                                   # :175
        PtsWithNorm1[:, 0:3] = (np.dot(R, PtsWithNorm1[:, 0:3].T) + T).T   # :176 (the normals stay)
        R_star = np.dot(R, R_star)
        T_star = np.dot(R, T_star) + T
        normEulers = np.linalg.norm(RotateMat2EulerAngle_XYZ(R))
        normT = np.linalg.norm(T)
        if trace is not None:
            trace.append((int(in0p.shape[0]), int(in0q.shape[0]), float(inlierThreshold0), float(inlierThreshold1)))
        converged = iIter >= minIterTimes and normEulers < ep and normT < ep   # :185-187
        if not converged and normEulers < smallShiftThreshold and normT < smallShiftThreshold:   # :190-192
            inlierThreshold0 *= decay_rate0
            inlierThreshold1 *= decay_rate1
        _icp_step(steps, iIter + 1, True, in0p.shape[0], in0q.shape[0], inlierThreshold0, inlierThreshold1, R_star, T_star,
                  min(margins), True)
        if converged:
            break
    return R_star, T_star, isSuccess


def GetRtFromOnePose(pose):
    """Transformations.py:164-168."""
    pose = np.asarray(pose).reshape(3, 4)
    return pose[:, 0:3], pose[:, 3].reshape(3, 1)


def GetRelRtBetween2Poses(pose0, pose1):
    """Transformations.py:106-113."""
    R0, T0 = GetRtFromOnePose(pose0)
    R0_inv = np.linalg.inv(R0)
    T0_inv = -np.dot(R0_inv, T0)
    R1, T1 = GetRtFromOnePose(pose1)
    return np.dot(R0_inv, R1), np.dot(R0_inv, T1) + T0_inv


def GetLidarRelRtBetween2Poses(pose0, pose1, R_Tr, T_Tr, R_Tr_inv, T_Tr_inv):
    """Transformations.py:118-125."""
    R0, T0 = GetRtFromOnePose(pose0)
    R0_inv = np.linalg.inv(R0)
    T0_inv = -np.dot(R0_inv, T0)
    R1, T1 = GetRtFromOnePose(pose1)
    R = np.dot(R_Tr_inv, np.dot(R0_inv, np.dot(R1, R_Tr)))
    T = np.dot(R_Tr_inv, np.dot(R0_inv, np.dot(R1, T_Tr) + T1) + T0_inv) + T_Tr_inv
    return R, T


def ForwardUpdatePoses(poses, frameNum, newPose, relRs, relTs):
    """RefinePoses.py:120-145."""
    poses_, relRs_, relTs_ = np.array(poses), np.array(relRs), np.array(relTs)
    poses_[frameNum, :] = newPose
    relR, relT = GetRelRtBetween2Poses(poses_[frameNum - 1, :], newPose)
    relRs_[frameNum - 1, :, :] = relR
    relTs_[frameNum - 1, :] = relT.reshape(3,)
    for iFrame in range(frameNum + 1, poses_.shape[0], 1):
        R0, T0 = GetRtFromOnePose(poses_[iFrame - 1])
        R = np.dot(R0, relRs_[iFrame - 1, :, :])
        T = np.dot(R0, relTs_[iFrame - 1, :].reshape(3, 1)) + T0
        poses_[iFrame, :] = np.c_[R, T].reshape((1, 12))
    return poses_, relRs_, relTs_


def RefinementCore(poses, ExtKeyPts0, PlanarPts0, ExtKeyPts1, PlanarPts1, iFrame0, iFrame1, relRs, relTs, inlierThreshold0, Tr,
                   icp=None, rng=None):
    """RefinePoses.py:273-334 with the two file reads (:276-277) replaced by their results (arrays) and the module
    globals R_Tr / T_Tr / ... (:549-556) derived from ``Tr``; ``icp`` = the ICP_Pt2PtAndPt2Plane to call (default: the
    restatement above)."""
    icp = icp or ICP_Pt2PtAndPt2Plane
    poses_ = np.array(poses)
    R_Tr, T_Tr = GetRtFromOnePose(np.asarray(Tr))
    R_Tr_inv = np.linalg.inv(R_Tr)
    T_Tr_inv = -np.dot(R_Tr_inv, T_Tr)
    pose0, pose1 = poses[iFrame0, :], poses[iFrame1, :]
    oriRelR, oriRelT = GetLidarRelRtBetween2Poses(pose0, pose1, R_Tr, T_Tr, R_Tr_inv, T_Tr_inv)        # :283
    KeyPts1_ = np.array(((np.dot(oriRelR, ExtKeyPts1.T) + oriRelT).T), dtype=np.float32)               # :284
    PlanarPts1_ = np.array(PlanarPts1)                                                                 # :286
    PlanarPts1_[:, 0:3] = np.array(((np.dot(oriRelR, PlanarPts1[:, 0:3].T) + oriRelT).T), dtype=np.float32)   # :287
    R_ICP, T_ICP, isSuccess = icp(ExtKeyPts0, KeyPts1_, PlanarPts0, PlanarPts1_, maxIterTimes=50, minIterTimes=20 - 1,
                                  inlierThreshold0=inlierThreshold0, decay_rate0=0.9, inlierThreshold1=5.0, decay_rate1=0.9,
                                  smallShiftThreshold=0.1, ep=0.001, **({"rng": rng} if rng is not None else {}))   # :290-293
    if isSuccess == False:                                                                             # :297-298
        return -1, poses_, relRs, relTs
    relativeR = np.dot(R_ICP, oriRelR)                                                                 # :300-301
    relativeT = np.dot(R_ICP, oriRelT) + T_ICP
    diffRelEulers = np.linalg.norm(RotateMat2EulerAngle_XYZ(oriRelR) - RotateMat2EulerAngle_XYZ(relativeR))   # :304-307
    diffRelT = np.linalg.norm(oriRelT - relativeT)
    if diffRelEulers > 10 or diffRelT > 5:                                                             # :308-309
        return 0, poses_, relRs, relTs
    R0, T0 = GetRtFromOnePose(pose0)                                                                   # :313
    R_poseDiff = np.dot(R_Tr, np.dot(relativeR, R_Tr_inv))                                             # :315-316
    T_poseDiff = np.dot(R_Tr, np.dot(relativeR, T_Tr_inv) + relativeT) + T_Tr
    R = np.dot(R0, R_poseDiff)
    T = np.dot(R0, T_poseDiff) + T0
    pose1 = np.c_[R, T].reshape((12,))                                                                 # :320-321
    poses_, relRs, relTs = ForwardUpdatePoses(poses, iFrame1, pose1, relRs, relTs)                     # :326
    return 1, poses_, relRs, relTs


def Voxelization(PC):
    """Voxel.py:100-173.  Returns the reference's 9-tuple; only AllVoxels0/1/2 (the members the
    hot path consumes) are populated, the block structures are None."""
    PC = np.ascontiguousarray(PC, dtype=np.float32)
    n, stride = PC.shape
    a0 = np.empty((n, 3), np.int16)
    a1 = np.empty((n, 3), np.int16)
    a2 = np.empty((n, 3), np.int16)
    cnt = np.zeros(3, np.int64)
    rc = lib().orc_voxelize(_p(PC), C.c_int64(n), C.c_int(stride), _p(a0), _p(a1), _p(a2), _p(cnt))
    if rc != 0:
        raise IndexError("voxel index out of bounds for its block")
    return (None, None, None, None, None, None,
            a0[:cnt[0]].copy(), a1[:cnt[1]].copy(), a2[:cnt[2]].copy())


def patches_bits(Pts, AllVoxels, scale):
    """One scale of GetPatchesList as bit-packed patches [K,64] u64 + flags [K] u8."""
    Pts = np.ascontiguousarray(Pts, dtype=np.float32)
    vox = np.ascontiguousarray(AllVoxels, dtype=np.int16)
    bits = np.zeros((Pts.shape[0], 64), dtype=np.uint64)
    flags = np.zeros(Pts.shape[0], dtype=np.uint8)
    rc = lib().orc_patches(_p(Pts), C.c_int64(Pts.shape[0]), _p(vox), C.c_int64(vox.shape[0]),
                           C.c_int(scale), _p(bits), _p(flags))
    if rc != 0:
        raise ValueError("Expected n_neighbors <= n_samples,  but n_samples = %d, n_neighbors = 496"
                         % vox.shape[0])
    return bits, flags


def argpartition(row, kth):
    """np.argpartition(row, kth) of NumPy 1.18 .. 1.26 (introselect) on one row of integers: the full index permutation [n] int32.
    scikit-learn's brute-force kneighbors (lists of fewer than 994 voxels at Voxel.py:195) keeps its first 496 entries."""
    v = np.ascontiguousarray(row, dtype=np.int64)
    out = np.empty(v.shape[0], np.int32)
    lib().orc_argpartition(_p(v), C.c_int64(v.shape[0]), C.c_int64(kth), _p(out))
    return out


def brute_query(AllVoxels, KeyVoxels):
    """kneighbors(KeyVoxels, 496) of the brute-force branch as SETS of list indices: [Q, 496] int32 (argpartition order)."""
    vox = np.ascontiguousarray(AllVoxels, dtype=np.int16)
    q = np.ascontiguousarray(KeyVoxels, dtype=np.int32)
    out = np.empty((q.shape[0], 496), np.int32)
    lib().orc_brute_query(_p(vox), C.c_int64(vox.shape[0]), _p(q), C.c_int64(q.shape[0]), _p(out))
    return out


def kdtree_idx(AllVoxels):
    """The index array of scikit-learn 0.24's KDTree(AllVoxels, leaf_size=30) (what NearestNeighbors(algorithm='auto') builds for
    n >= 994 at Voxel.py:195): (idx [n] int32, n_nodes).  tools/make_goldens.py compares it with KDTree.get_arrays()[1]."""
    vox = np.ascontiguousarray(AllVoxels, dtype=np.int16)
    idx = np.empty(vox.shape[0], np.int32)
    n_nodes = lib().orc_kdtree_idx(_p(vox), C.c_int64(vox.shape[0]), _p(idx))
    return idx, int(n_nodes)


def kdtree_work(AllVoxels):
    """The device build's work budget on this list (csrc/kdorder.hip), restated serially: (the largest quickselect work of a node in
    passes' worth of its length -- the budget is 4096 of them plus 65536 elements --, whether any node runs past it: the device
    would abandon the tree).  Only chooses and checks test lists."""
    vox = np.ascontiguousarray(AllVoxels, dtype=np.int16)
    w = C.c_double(0.0)
    over = lib().orc_kdtree_work(_p(vox), C.c_int64(vox.shape[0]), C.byref(w))
    return float(w.value), bool(over)


def kdtree_query(AllVoxels, KeyVoxels):
    """kneighbors(KeyVoxels, 496) of that tree as SETS of list indices: [Q, 496] int32 (heap order, not sorted)."""
    vox = np.ascontiguousarray(AllVoxels, dtype=np.int16)
    q = np.ascontiguousarray(KeyVoxels, dtype=np.int32)
    out = np.empty((q.shape[0], 496), np.int32)
    lib().orc_kdtree_query(_p(vox), C.c_int64(vox.shape[0]), _p(q), C.c_int64(q.shape[0]), _p(out))
    return out


def unpack_patches(bits):
    """[K,64] u64 -> [K,16,16,16,1] f32 (the reference's dense layout)."""
    b = np.ascontiguousarray(bits, dtype="<u8").view(np.uint8).reshape(bits.shape[0], 512)
    d = np.unpackbits(b, axis=1, bitorder="little")
    return d.reshape(bits.shape[0], 16, 16, 16, 1).astype(np.float32)


def pack_patches(dense):
    """[K,16,16,16(,1)] {0,1} -> [K,64] u64."""
    d = (np.asarray(dense).reshape(dense.shape[0], 4096) != 0).astype(np.uint8)
    return np.packbits(d, axis=1, bitorder="little").view("<u8").reshape(dense.shape[0], 64)


def GetPatchesList(Pts, AllVoxels0, AllVoxels1, AllVoxels2, return_flags=False):
    """Voxel.py:177-216 -> (Pts, [P0,P1,P2]) with P_s [K,16,16,16,1] f32."""
    out, flags = [], []
    for s, vox in enumerate((AllVoxels0, AllVoxels1, AllVoxels2)):
        b, f = patches_bits(Pts, vox, s)
        out.append(unpack_patches(b))
        flags.append(f)
    return (Pts, out, flags) if return_flags else (Pts, out)


class _EncW(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("w1", "b1", "w2", "b2", "w3", "b3", "wd1", "bd1", "wd2", "bd2")]


class PatchEncoder:
    """Stand-in for keras ``load_model(EncoderModel4VoxelPatch.h5)`` (all-tanh)."""

    def __init__(self, weights):
        self.w = [np.ascontiguousarray(a, np.float32) for a in weights]
        assert [a.size for a in self.w] == [216, 8, 3456, 16, 13824, 32, 409600, 200, 4000, 20]
        self._s = _EncW(*[a.ctypes.data for a in self.w])

    def predict_bits(self, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        out = np.empty((bits.shape[0], 20), dtype=np.float32)
        lib().orc_encode(_p(bits), C.c_int64(bits.shape[0]), C.byref(self._s), _p(out),
                         C.c_int(20), C.c_int(0))
        return out

    def predict(self, patches):
        return self.predict_bits(pack_patches(patches))

    def predict_layers(self, bits):
        """-> (p2 [K,1024] after pool2, f3 [K,2048] after conv3, h [K,200] after Dense(200), out [K,20]): the activations
        between the HIP encoder's kernels, for the per-layer error budget test."""
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        k = bits.shape[0]
        p2, f3, h, out = (np.empty((k, d), dtype=np.float32) for d in (1024, 2048, 200, 20))
        lib().orc_encode_layers(_p(bits), C.c_int64(k), C.byref(self._s), _p(out), C.c_int(20), _p(p2), _p(f3), _p(h))
        return p2, f3, h, out


# ---- BASELINE.json configs[4]: 32^3 patches (not a reference code path; see caelo_oracle.c) ----------
def patches32_bits(Pts, AllVoxels, scale):
    """Config 5: GetPatchesList's rule (Voxel.py:177-216) with PatchSize=32 and the 496-NN cap disabled ->
    bit-packed patches [K,512] u64, lin = (ix*32+iy)*32+iz at bit lin&63 of word lin>>6."""
    Pts = np.ascontiguousarray(Pts, dtype=np.float32)
    vox = np.ascontiguousarray(AllVoxels, dtype=np.int16)
    bits = np.zeros((Pts.shape[0], 512), dtype=np.uint64)
    lib().orc_patches32(_p(Pts), C.c_int64(Pts.shape[0]), _p(vox), C.c_int64(vox.shape[0]), C.c_int(scale),
                        _p(bits))
    return bits


def unpack_patches32(bits):
    """[K,512] u64 -> [K,32,32,32,1] f32."""
    b = np.ascontiguousarray(bits, dtype="<u8").view(np.uint8).reshape(bits.shape[0], 4096)
    return np.unpackbits(b, axis=1, bitorder="little").reshape(bits.shape[0], 32, 32, 32, 1).astype(np.float32)


class PatchEncoder32:
    """Config-5 encoder: PatchEncoder's conv kernels, biases and dense_2 with ``dense1`` [16384,200] as the
    first dense layer (seeded stand-in -- no trained weights exist at this size)."""

    def __init__(self, weights, dense1, bias1):
        self.w = [np.ascontiguousarray(a, np.float32) for a in weights]
        self.w[6] = np.ascontiguousarray(dense1, np.float32)
        self.w[7] = np.ascontiguousarray(bias1, np.float32)
        assert self.w[6].shape == (16384, 200) and self.w[7].shape == (200,)
        self._s = _EncW(*[a.ctypes.data for a in self.w])

    def predict_bits(self, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        assert bits.shape[1] == 512
        out = np.empty((bits.shape[0], 20), dtype=np.float32)
        lib().orc_encode32(_p(bits), C.c_int64(bits.shape[0]), C.byref(self._s), _p(out), C.c_int(20), C.c_int(0))
        return out


def GetFeaturesFromPatches(PatchEncoder_, PatchesList):
    """Match.py:130-135."""
    return np.c_[PatchEncoder_.predict(PatchesList[0]), PatchEncoder_.predict(PatchesList[1]),
                 PatchEncoder_.predict(PatchesList[2])]


# What orc_respond / orc_encode restate (the .h5's model_config): (class, filters-or-units, kernel, activation).
# Kept apart from caelo.keras_config on purpose: the checker must not lean on the package under test.
_RESPOND_STACK = [("Conv2D", 32, [3, 3], "relu"), ("Conv2D", 8, [1, 1], "relu")]
_ENCODER_STACK = [("Conv3D", 8, [3, 3, 3], "tanh"), ("MaxPooling3D", None, [2, 2, 2], None), ("Conv3D", 16, [3, 3, 3], "tanh"),
                  ("MaxPooling3D", None, [2, 2, 2], None), ("Conv3D", 32, [3, 3, 3], "tanh"), ("Flatten", None, None, None),
                  ("Dense", 200, None, "tanh"), ("Dense", 20, None, "tanh")]


def _check_stack(h5, want):
    import json
    cfg = json.loads(h5.attrs("/")["model_config"].decode("utf8"))["config"]
    got = []
    for l in (cfg["layers"] if isinstance(cfg, dict) else cfg):
        c = l["config"]
        if l["class_name"] == "InputLayer":
            continue
        if l["class_name"].startswith("Conv") and (c["padding"] != "same" or list(c["strides"]) != [1] * len(c["strides"])
                                                   or c.get("data_format", "channels_last") != "channels_last" or not c["use_bias"]):
            raise ValueError("oracle: unsupported convolution %s" % c)
        got.append((l["class_name"], c.get("filters", c.get("units")),
                    list(c["kernel_size"]) if "kernel_size" in c else (list(c["pool_size"]) if "pool_size" in c else None),
                    c.get("activation")))
    if got != want:
        raise ValueError("oracle: the .h5 holds %s, the restatement implements %s" % (got, want))


def load_models(respond_h5, encoder_h5):
    """Read both Keras .h5 files (through caelo.h5lite -- file parsing only, no compute)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "cae-lo_amd"))
    from caelo.h5lite import H5File   # HDF5 container parsing only; the layer-stack check below is the oracle's own
    for path, want in ((respond_h5, _RESPOND_STACK), (encoder_h5, _ENCODER_STACK)):   # the restatement IS this stack: refuse others
        _check_stack(H5File(path), want)
    r = H5File(respond_h5)
    g = lambda h, l, n: h.dataset("/model_weights/%s/%s/%s:0" % (l, l, n))
    resp = RespondLayer(g(r, "conv2d_1", "kernel"), g(r, "conv2d_1", "bias"),
                        g(r, "conv2d_2", "kernel"), g(r, "conv2d_2", "bias"))
    e = H5File(encoder_h5)
    ws = []
    for l in ("conv3d_1", "conv3d_2", "conv3d_3", "dense_1", "dense_2"):
        ws += [g(e, l, "kernel"), g(e, l, "bias")]
    return resp, PatchEncoder(ws)


# ---------------------------------------------------------------------------------------------
def match(Codes0, Codes1):
    """Match.py:257-258: argmin over frame-0 descriptors for every frame-1 keypoint (f64)."""
    f0 = np.ascontiguousarray(Codes0, np.float32)
    f1 = np.ascontiguousarray(Codes1, np.float32)
    idx = np.empty(f1.shape[0], np.int64)
    dist = np.empty(f1.shape[0], np.float64)
    lib().orc_match(_p(f0), C.c_int64(f0.shape[0]), _p(f1), C.c_int64(f1.shape[0]),
                    C.c_int(f0.shape[1]), _p(idx), _p(dist))
    return idx, dist


def SolveRT(Pairs0, Pairs1):
    """Match.py:138-158 (same NumPy/LAPACK calls, incl. the Vh column flip at :154)."""
    isCredible = 1
    mean0 = np.mean(Pairs0, axis=0).reshape(1, 3)
    mean1 = np.mean(Pairs1, axis=0).reshape(1, 3)
    P0 = Pairs0 - mean0
    P1 = Pairs1 - mean1
    H = np.dot(P1.T, P0)
    U, S, V = np.linalg.svd(H)
    R = np.dot(V.T, U.T)
    if np.linalg.det(R) < 0:
        isCredible = -1
        V[:, 2] = V[:, 2] * (-1)
        R = np.dot(V.T, U.T)
    T = mean0.T - np.dot(R, mean1.T)
    return R, T, isCredible


def draw_sample_indices(rng, n_pairs):
    """The 4 indices one RANSAC iteration consumes (Match.py:182-184)."""
    return np.array(rng.random_sample((4,)) * n_pairs, dtype=np.int32)


def RANSAC4RT(Pairs0, Pairs1, Weights0=None, Weights1=None, rng=None, trace=None):
    """Match.py:162-218.  ``rng``: a ``np.random.RandomState`` standing for the reference's
    global NumPy RNG (``np.random.seed(s)`` before the call == ``RandomState(s)`` here)."""
    if rng is None:
        rng = np.random.mtrand._rand
    N = Pairs0.shape[0]
    leastInliers = min(100, int(0.2 * N))
    minSuccessInliers = 0.25 * N
    minTrails, maxTrails = 100, 500
    residualThreshold = 0.4
    isSuccess = False
    cntIters = 0
    curNumInliers = 0
    R_star = np.eye(3, dtype=np.float64)
    T_star = np.zeros((3, 1), dtype=np.float64)
    inlierIdx_star = np.zeros((N,), dtype=bool)
    while True:
        while (cntIters < minTrails) or (cntIters >= minTrails and cntIters < maxTrails
                                         and curNumInliers < minSuccessInliers):
            RandIdxes = draw_sample_indices(rng, N)
            R, T, _ = SolveRT(Pairs0[RandIdxes, :], Pairs1[RandIdxes, :])
            Pairs1_ = (np.dot(R, Pairs1.T) + T).T
            dists = np.linalg.norm(Pairs0 - Pairs1_, axis=1)
            inlierIdx = dists < residualThreshold
            nInliers = int(inlierIdx.sum())
            if trace is not None:
                trace.append((RandIdxes.copy(), nInliers, float(residualThreshold)))
            if nInliers < leastInliers:
                cntIters += 1
                continue
            if nInliers > curNumInliers:
                curNumInliers = nInliers
                inlierIdx_star = inlierIdx
                R_star, T_star = R, T
            cntIters += 1
            isSuccess = True
        if isSuccess:
            break
        cntIters = 0
        residualThreshold = 2 * residualThreshold
        if residualThreshold > 2.0:
            residualThreshold = residualThreshold / 2
            break
    return R_star, T_star, isSuccess, inlierIdx_star, residualThreshold


def SolveRelativePose(OriPC0, OriCodes0, Weights0, OriPC1, OriCodes1, Weights1, rng=None,
                      trace=None):
    """Match.py:241-283."""
    pairIdx, _ = match(OriCodes0, OriCodes1)
    Pairs0 = OriPC0[pairIdx, :]
    Pairs1 = OriPC1
    idxPairs1 = np.arange(OriPC1.shape[0])
    R, T, isSuccess, inlierIdx, thr = RANSAC4RT(Pairs0, Pairs1, None, None, rng=rng, trace=trace)
    inliersIdx0 = pairIdx[inlierIdx]
    inliersIdx1 = idxPairs1[inlierIdx]
    if inliersIdx0.shape[0] == 0:
        return R, T, isSuccess, inliersIdx0, inliersIdx1, thr
    R, T, _ = SolveRT(OriPC0[inliersIdx0, :], OriPC1[inliersIdx1, :])
    return R, T, isSuccess, inliersIdx0, inliersIdx1, thr
