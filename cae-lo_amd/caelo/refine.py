"""Host side of the pose refinement that follows the odometry: the 3 x 4 pose algebra of
Transformations.py and the control flow of RefinePoses.RefinementCore.  The registration itself (ICP_Pt2PtAndPt2Plane)
runs on the device (caelo_icp, csrc/icp.hip) and is passed in."""
import math

import numpy as np


def RotateMat2EulerAngle_XYZ(R):
    """Transformations.py:181-186 (degrees)."""
    return np.array([math.atan2(R[2, 1], R[2, 2]), math.atan2(-R[2, 0], math.sqrt(R[2, 1] ** 2 + R[2, 2] ** 2)),
                     math.atan2(R[1, 0], R[0, 0])]) * (180.0 / math.pi)


def GetRtFromOnePose(pose):
    """Transformations.py:164-168: a KITTI 12-float row -> (R [3,3], T [3,1])."""
    m = np.asarray(pose).reshape(3, 4)
    return m[:, 0:3], m[:, 3].reshape(3, 1)


def GetRelRtBetween2Poses(pose0, pose1):
    """Transformations.py:106-113: motion from pose0 to pose1 in the frame of pose0."""
    Ra, Ta = GetRtFromOnePose(pose0)
    Ra_inv = np.linalg.inv(Ra)
    Rb, Tb = GetRtFromOnePose(pose1)
    return Ra_inv @ Rb, Ra_inv @ Tb - Ra_inv @ Ta


def GetLidarRelRtBetween2Poses(pose0, pose1, R_Tr, T_Tr, R_Tr_inv, T_Tr_inv):
    """Transformations.py:118-125: the same motion expressed in the LiDAR frame (camera poses conjugated by Tr)."""
    Ra, Ta = GetRtFromOnePose(pose0)
    Ra_inv = np.linalg.inv(Ra)
    Rb, Tb = GetRtFromOnePose(pose1)
    R = R_Tr_inv @ (Ra_inv @ (Rb @ R_Tr))
    T = R_Tr_inv @ (Ra_inv @ (Rb @ T_Tr + Tb) - Ra_inv @ Ta) + T_Tr_inv
    return R, T


def ForwardUpdatePoses(poses, frameNum, newPose, relRs, relTs):
    """RefinePoses.py:120-145: frame ``frameNum`` takes ``newPose``; the poses after it are re-chained from the stored
    relative motions; the relative motion into frameNum is recomputed.  Inputs are not modified."""
    out_poses, out_Rs, out_Ts = np.array(poses), np.array(relRs), np.array(relTs)
    out_poses[frameNum, :] = newPose
    dR, dT = GetRelRtBetween2Poses(out_poses[frameNum - 1, :], newPose)
    out_Rs[frameNum - 1, :, :] = dR
    out_Ts[frameNum - 1, :] = dT.reshape(3,)
    for k in range(frameNum + 1, out_poses.shape[0]):
        Rp, Tp = GetRtFromOnePose(out_poses[k - 1])
        out_poses[k, :] = np.c_[Rp @ out_Rs[k - 1], Rp @ out_Ts[k - 1].reshape(3, 1) + Tp].reshape(12)
    return out_poses, out_Rs, out_Ts


def RefinementCore(poses, ExtKeyPts0, PlanarPts0, ExtKeyPts1, PlanarPts1, iFrame0, iFrame1, relRs, relTs, inlierThreshold0, Tr, icp, rng=None):
    """RefinePoses.py:273-334.  flag: -1 registration failed, 0 rejected (the relative pose would change by more than
    10 degrees or 5 m), 1 pose of iFrame1 refined and the later poses forward-updated."""
    untouched = np.array(poses)
    R_Tr, T_Tr = GetRtFromOnePose(np.asarray(Tr))
    R_Tr_inv = np.linalg.inv(R_Tr)
    T_Tr_inv = -(R_Tr_inv @ T_Tr)
    pose_a, pose_b = poses[iFrame0, :], poses[iFrame1, :]
    odoR, odoT = GetLidarRelRtBetween2Poses(pose_a, pose_b, R_Tr, T_Tr, R_Tr_inv, T_Tr_inv)                 # :283
    moved = np.array((odoR @ np.asarray(ExtKeyPts1).T + odoT).T, dtype=np.float32)                          # :284
    planar_moved = np.array(PlanarPts1)
    planar_moved[:, 0:3] = np.array((odoR @ np.asarray(PlanarPts1)[:, 0:3].T + odoT).T, dtype=np.float32)   # :286-287
    R_icp, T_icp, ok = icp(ExtKeyPts0, moved, PlanarPts0, planar_moved, maxIterTimes=50, minIterTimes=20 - 1,
                           inlierThreshold0=inlierThreshold0, decay_rate0=0.9, inlierThreshold1=5.0, decay_rate1=0.9,
                           smallShiftThreshold=0.1, ep=0.001, rng=rng)                                      # :290-293
    if not ok:
        return -1, untouched, relRs, relTs                                                                  # :297-298
    newR, newT = R_icp @ odoR, R_icp @ odoT + T_icp                                                         # :300-301
    d_euler = np.linalg.norm(RotateMat2EulerAngle_XYZ(odoR) - RotateMat2EulerAngle_XYZ(newR))              # :304-306
    if d_euler > 10 or np.linalg.norm(odoT - newT) > 5:                                                     # :307-309
        return 0, untouched, relRs, relTs
    Ra, Ta = GetRtFromOnePose(pose_a)
    camR = R_Tr @ (newR @ R_Tr_inv)                                                                         # :315
    camT = R_Tr @ (newR @ T_Tr_inv + newT) + T_Tr                                                           # :316
    refined = np.c_[Ra @ camR, Ra @ camT + Ta].reshape(12)                                                  # :317-321
    out = ForwardUpdatePoses(poses, iFrame1, refined, relRs, relTs)                                         # :326
    return (1,) + out


# ---- the sequence logic of RefinePoses.py: de-jump, the refinement walk, the second pass ---------------------------
# The walks take the registration as a callable ``core(poses, iFrame0, iFrame1, relRs, relTs, inlierThreshold0) -> (code, poses,
# relRs, relTs)`` -- RefinementCore with the key points and the ICP bound (``make_core``) -- and the inlier pairs of two consecutive
# frames as a callable ``pairs(f0, f1) -> (inliersIdx0, inliersIdx1)``, so they run without a device or files.
def GetRelRsAndTs(poses):
    """Transformations.py:94-103: the relative motion between every two consecutive poses -> (RelRs [n-1,3,3], RelTs [n-1,3]) f64."""
    n = poses.shape[0]
    RelRs = np.zeros((n - 1, 3, 3), dtype=np.float64)
    RelTs = np.zeros((n - 1, 3), dtype=np.float64)
    for iFrame in range(n - 1):
        R, T = GetRelRtBetween2Poses(poses[iFrame, :], poses[iFrame + 1, :])
        RelRs[iFrame, :, :] = R
        RelTs[iFrame, :] = T.reshape(1, 3)
    return RelRs, RelTs


def ConvertRelRsIntoEulers(relRs):
    """Transformations.py:170-174."""
    Eulers = np.zeros((relRs.shape[0], 3), dtype=np.float64)
    for i in range(relRs.shape[0]):
        Eulers[i, :] = RotateMat2EulerAngle_XYZ(relRs[i, :, :])
    return Eulers


def GetDiffRels(poses):
    """Transformations.py:83-92: -> (RelRs, RelTs, RelEulers, diffRelEulers [n-2], diffRelTs [n-2]); the differences are taken
    between the ABSOLUTE values of consecutive relative motions (:85-86)."""
    RelRs, RelTs = GetRelRsAndTs(poses)
    RelEulers = ConvertRelRsIntoEulers(RelRs)
    diffRelEulers = np.linalg.norm(np.abs(RelEulers[1:RelEulers.shape[0], :]) - np.abs(RelEulers[0:RelEulers.shape[0] - 1, :]), axis=1)
    diffRelTs = np.linalg.norm(np.abs(RelTs[1:RelTs.shape[0], :]) - np.abs(RelTs[0:RelTs.shape[0] - 1, :]), axis=1)
    return RelRs, RelTs, RelEulers, diffRelEulers, diffRelTs


def FixJumpPoses(poses, log=None):
    """RefinePoses.py:233-262: a frame whose relative motion differs from the one before it by more than 2.0 degrees or 0.5 m repeats
    that motion instead; the later poses are re-chained and the differences recomputed after every fix.  -> (poses, deJumpedFrames)
    (the reference prints the list and returns the poses alone)."""
    poses_ = np.array(poses)
    relRs, relTs, relEulers, diffNormRelEulers, diffNormRelTs = GetDiffRels(poses_)
    EulersThreshold = 2.0  # degree
    TsThreshold = 0.5
    deJumpedFrames = []
    for iFrame in range(2, poses_.shape[0] - 1, 1):                                                        # :242
        if diffNormRelEulers[iFrame - 2] > EulersThreshold or diffNormRelTs[iFrame - 2] > TsThreshold:     # :243
            prevRelR = relRs[iFrame - 2, :, :]
            prevRelT = relTs[iFrame - 2, :].reshape(3, 1)
            R0, T0 = GetRtFromOnePose(poses_[iFrame - 1])
            newPose = np.c_[R0 @ prevRelR, R0 @ prevRelT + T0].reshape(12)                                 # :251-254
            poses_, relRs, relTs = ForwardUpdatePoses(poses_, iFrame, newPose, relRs, relTs)               # :256
            if log:
                log("fixed jump pose at %d" % iFrame)
            deJumpedFrames.append(iFrame)
            relRs, relTs, relEulers, diffNormRelEulers, diffNormRelTs = GetDiffRels(poses_)                # :260
    return poses_, deJumpedFrames


def GetTransferPairIdx(idx0, idx1):
    """RefinePoses.py:102-114: for every entry i of idx0 whose value occurs in idx1, [i, first position of that value in idx1]
    (cdist of the doubled columns is 0 exactly where the values are equal, and argmin keeps the first zero).  idx1 may hold a value
    more than once.  The distance matrix is not built."""
    idx0, idx1 = np.asarray(idx0).reshape(-1), np.asarray(idx1).reshape(-1)
    if idx0.shape[0] < 1 or idx1.shape[0] < 1:
        return []
    first = {}
    for pos, v in enumerate(idx1.tolist()):
        first.setdefault(v, pos)
    return [[i, first[v]] for i, v in enumerate(idx0.tolist()) if v in first]


def LongestPair(pairs, iFrame, nFrames, nMaxTransferFrames, nMinTransferPairs=1):
    """RefinePoses.py:375-400: starting from the inlier pairs of (iFrame, iFrame + 1), follow the key points that stay inliers
    from pair to pair -> [iFrame0, iFrame1, idx0, idx1], the longest span some key point survives (at most nMaxTransferFrames)."""
    idx0, idx1 = pairs(iFrame, iFrame + 1)
    cur = [iFrame, iFrame + 1, np.asarray(idx0).reshape(-1), np.asarray(idx1).reshape(-1)]
    while cur[3].shape[0] > nMinTransferPairs:                                                             # :382 (strict)
        iFrame0 = cur[1]
        iFrame1 = cur[1] + 1
        if iFrame1 >= nFrames - 1:                                                                         # :385
            break
        Idx0, Idx1 = pairs(iFrame0, iFrame1)
        Idx0, Idx1 = np.asarray(Idx0).reshape(-1), np.asarray(Idx1).reshape(-1)
        transferedIdxes = GetTransferPairIdx(cur[3], Idx0)
        if len(transferedIdxes) < nMinTransferPairs or cur[1] - cur[0] >= nMaxTransferFrames:             # :394
            break
        transferedIdxes = np.array(transferedIdxes)
        cur[1] = iFrame1
        cur[2] = cur[2][transferedIdxes[:, 0]]
        cur[3] = Idx1[transferedIdxes[:, 1]]
    return cur


def ComputeErrorsofRT(R_GT, T_GT, R_Estimated, T_Estimated):
    """RefinePoses.py:467-473 -> (sum |error Euler angles| in degrees, sum |error T|)."""
    eulers_error = RotateMat2EulerAngle_XYZ(np.linalg.inv(R_GT) @ R_Estimated)
    T_error = T_Estimated - T_GT
    return np.sum(np.abs(eulers_error.reshape(1, 3))), np.sum(np.abs(T_error.reshape(1, 3)))


def RefineOdometry(poses__, iOption, core, pairs=None, gt=None, iStartFrame=0, log=None):
    """RefinePoses.py:338-464.  iOption 0: every consecutive pair; 1: key frames by inlier transfer (``pairs`` needed).  ``gt``: the
    ground-truth poses or None (the reference's iGroundTruth).  -> (poses___, aDebugInfo float32, failedFrames, tried): aDebugInfo
    rows are [f0, f1, sum|T_GT|, RRE_ori, RTE_ori, RRE_after, RTE_after] with ground truth and [f0, f1, deltaAngle, deltaT] without;
    ``tried`` lists every (f0, f1, code) in order (the reference prints them)."""
    poses___ = np.array(poses__)
    relRs, relTs, relEulers, diffNormRelEulers, diffNormRelTs = GetDiffRels(poses___)
    nMinTransferPairs = 1
    nMaxTransferFrames_bkp = 20
    nMaxTransferFrames = nMaxTransferFrames_bkp
    iFrame = iStartFrame
    iEndFrame = poses___.shape[0] - 2                                                                      # :361
    failedFrames, tried, debugInfo = [], [], []
    while iFrame < iEndFrame:
        if iOption == 0:
            cur = [iFrame, iFrame + 1]                                                                     # :371-373
        else:
            cur = LongestPair(pairs, iFrame, poses___.shape[0], nMaxTransferFrames, nMinTransferPairs)
        reCode, poses___, relRs, relTs = core(poses___, cur[0], cur[1], relRs, relTs, 1.0)               # :405
        tried.append((int(cur[0]), int(cur[1]), int(reCode)))
        if reCode == -1 or reCode == 0:                                                                    # :411-431
            if cur[1] - cur[0] > 1:
                if log:
                    log("%d - %d refine code %d, frame length = %d: the same start frame again, one frame" % (cur[0], cur[1], reCode, cur[1] - cur[0]))
                nMaxTransferFrames = 1  # iFrame stays the same
                continue
            if log:
                log("%d - %d refine failed%s" % (cur[0], cur[1], "" if reCode == -1 else " (unreliable)"))
            failedFrames.append([cur[0], cur[1]])
            nMaxTransferFrames = nMaxTransferFrames_bkp
            iFrame += 1
            continue
        iFrame = cur[1]                                                                                    # :434
        if log:
            log("%d - %d refine success, frame length = %d" % (cur[0], cur[1], cur[1] - cur[0]))
        nMaxTransferFrames = nMaxTransferFrames_bkp
        R_poseDiff_ori, T_poseDiff_ori = GetRelRtBetween2Poses(poses__[cur[0]], poses__[cur[1]])          # :440
        R_poseDiff, T_poseDiff = GetRelRtBetween2Poses(poses___[cur[0]], poses___[cur[1]])                # :441
        if gt is not None:
            R_GT, T_GT = GetRelRtBetween2Poses(gt[cur[0]], gt[cur[1]])
            RRE_ori, RTE_ori = ComputeErrorsofRT(R_GT, T_GT, R_poseDiff_ori, T_poseDiff_ori)
            RRE_after, RTE_after = ComputeErrorsofRT(R_GT, T_GT, R_poseDiff, T_poseDiff)
            debugInfo.append([cur[0], cur[1], np.sum(np.abs(T_GT.reshape(1, 3))), RRE_ori, RTE_ori, RRE_after, RTE_after])   # :448
        else:
            eulers_delta = RotateMat2EulerAngle_XYZ(np.linalg.inv(R_poseDiff_ori) @ R_poseDiff)          # :450-451
            T_delta = T_poseDiff - T_poseDiff_ori
            debugInfo.append([cur[0], cur[1], np.sum(np.abs(eulers_delta.reshape(1, 3))), np.sum(np.abs(T_delta.reshape(1, 3)))])   # :456
    return poses___, np.array(debugInfo, dtype=np.float32), failedFrames, tried


def CloseLoopPipeline(poses, refinementInfo, core, log=None):
    """RefinePoses.py:477-518, the second pass: the key frames are column 0 of the refinement's debug table; key frames k and k + 2
    are registered with threshold 0.5, k advancing by 2, while k + 2 < nKeyFrames - 5.  -> (poses, tried).  With 7 key frames or
    fewer nothing is registered; the reference raises IndexError below 3 key frames (:490-491), here the poses come back unchanged."""
    info = np.asarray(refinementInfo)
    poses_ = np.array(poses)
    tried = []
    if info.ndim != 2 or info.shape[0] < 3:
        return poses_, tried
    KeyFrames = np.array(info[:, 0], dtype=np.int32)
    nKeyFrames = KeyFrames.shape[0]
    relRs, relTs, relEulers, diffNormRelEulers, diffNormRelTs = GetDiffRels(poses_)
    iKeyFrame0 = 0
    iKeyFrame1 = 2
    iFrame0 = KeyFrames[iKeyFrame0]
    iFrame1 = KeyFrames[iKeyFrame1]
    while iKeyFrame1 < nKeyFrames - 5:                                                                     # :494
        reCode, poses_, relRs, relTs = core(poses_, int(iFrame0), int(iFrame1), relRs, relTs, 0.5)        # :497
        tried.append((int(iFrame0), int(iFrame1), int(reCode)))
        if log:
            log("%d - %d refine code %d frame length = %d" % (iFrame0, iFrame1, reCode, iFrame1 - iFrame0))
        iKeyFrame0 += 2                                                                                    # :513-516
        iKeyFrame1 = iKeyFrame0 + 2
        iFrame0 = KeyFrames[iKeyFrame0]
        iFrame1 = KeyFrames[iKeyFrame1]
    return poses_, tried


def pt2pt_adapter(ICP):
    """The reference's own alternative at RefinePoses.py:295, literally ``ICP(KeyPts0, KeyPts1_)`` with MyICP.ICP's defaults, in the
    shape RefinementCore calls its registration: the planar sets and the keyword arguments of :291-294 are ignored."""
    def icp(KeyPts0, KeyPts1_, PlanarPts0, PlanarPts1_, **ignored):
        return ICP(KeyPts0, KeyPts1_)
    return icp


def make_core(keypts, Tr, icp, seed_base=None, per_pair=False):
    """RefinementCore with its inputs bound -> the ``core`` callable of the walks.  ``keypts(frame) -> (ExtKeyPts [n,3] f32,
    PlanarPts [m,6] f32)`` (LoadExtendedKeyPts, :276-277); ``icp`` as RefinementCore takes it, or with ``per_pair`` a callable
    ``(iFrame0, iFrame1) ->`` such a registration (one that keeps frame iFrame0's points resident, say).  With ``seed_base`` the k-th
    call (k = 0, 1, ...) hands RandomState(seed_base + k) to the registration (the subsample of more than 2 000 planar points)."""
    calls = [0]

    def core(poses, iFrame0, iFrame1, relRs, relTs, inlierThreshold0):
        rng = None if seed_base is None else np.random.RandomState(seed_base + calls[0])
        calls[0] += 1
        KeyPts0, PlanarPts0 = keypts(iFrame0)
        KeyPts1, PlanarPts1 = keypts(iFrame1)
        return RefinementCore(poses, KeyPts0, PlanarPts0, KeyPts1, PlanarPts1, iFrame0, iFrame1, relRs, relTs, inlierThreshold0, Tr,
                              icp(iFrame0, iFrame1) if per_pair else icp, rng=rng)
    return core
