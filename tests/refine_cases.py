"""What tools/make_goldens_refine.py and tests/test_refine_sequence_host.py share: the scripted stand-in for RefinementCore and the
names of the cases of tests/golden/refine_sequence.npz.  The stand-in is handed the pose algebra it should use -- the reference's
own functions in the tool, caelo.refine's in the test -- so that both sides run the same script around their own arithmetic."""
import numpy as np

# refinement cases: name -> (sequence, iOption, with ground truth, iStartFrame)
WALKS = {
    "keyframes_gt": (2, 1, True, 0),
    "keyframes_nogt": (1, 1, False, 3),
    "consecutive_gt": (0, 0, True, 0),
    "consecutive_nogt": (1, 0, False, 0),
}
REAL = "real_icp"           # sequence 0, key frames, ground truth, the reference's ICP on small clouds
DEJUMP = ("rotation", "translation", "both", "frame_2", "frame_n_2", "two_in_a_row", "none")


def code_table(n):
    """The script: code[f0, f1] that the stand-in returns for the pair (f0, f1).  Long pairs and one-frame pairs each meet -1, 0
    and 1."""
    codes = np.ones((n, n), dtype=np.int8)
    for f0 in range(n):
        for f1 in range(f0 + 1, n):
            if f1 - f0 > 1:
                codes[f0, f1] = -1 if f0 % 7 == 0 else (0 if f0 % 7 == 3 else 1)
            else:
                codes[f0, f1] = -1 if f0 % 5 == 1 else (0 if f0 % 5 == 3 else 1)
    return codes


def scripted_core(codes, gt, ForwardUpdatePoses, GetRelRtBetween2Poses, GetRtFromOnePose, calls):
    """-> core(poses, iFrame0, iFrame1, relRs, relTs, inlierThreshold0) with RefinementCore's returns: the scripted code, and with
    code 1 frame iFrame1 placed at the ground truth's relative motion from iFrame0, the later poses forward-updated.  Every call
    is appended to ``calls`` as (iFrame0, iFrame1, inlierThreshold0)."""
    def core(poses, iFrame0, iFrame1, relRs, relTs, inlierThreshold0):
        calls.append((int(iFrame0), int(iFrame1), float(inlierThreshold0)))
        code = int(codes[iFrame0, iFrame1])
        if code != 1:
            return code, np.array(poses), relRs, relTs
        R, T = GetRelRtBetween2Poses(gt[iFrame0], gt[iFrame1])
        R0, T0 = GetRtFromOnePose(poses[iFrame0])
        pose1 = np.c_[np.dot(R0, R), np.dot(R0, T) + T0].reshape((12,))
        poses_, relRs_, relTs_ = ForwardUpdatePoses(poses, iFrame1, pose1, relRs, relTs)
        return 1, poses_, relRs_, relTs_
    return core
