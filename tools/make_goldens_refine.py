#!/opt/conda/bin/python3.9
"""Generate tests/golden/refine_sequence.npz from the reference's RefinePoses.py (read-only reference tree, see make_goldens.py).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tools/make_goldens_refine.py

Interpreter: the conda python3.9 (NumPy 1.26, scikit-learn 0.24.2), like tools/make_goldens_evaluate.py.  The function definitions
(and imports) of RefinePoses.py are loaded from the file at run time; its module-level script does not execute.  The globals its
functions read (PairsDir, strDataBaseDir, iGroundTruth, R_Tr ...) are set per run the way the script's loop sets them (:541-554).

A small KITTI-shaped tree is written to a temporary directory: 3 sequences of 14, 22 and 30 frames, ground truth on
synth.sensor_pose(trajectory="circuit"), estimates with a small chained error, a non-identity Tr, InliersIdx files (key point
tracks that die after 1, 3, 5 and 25 frames, duplicated inliersIdx0 entries in front of and behind the first occurrence, one empty
pair file), and for sequence 0 KeyPts files with 400 extended key points of a static world.

  * FixJumpPoses on estimates with planted jumps (tests/refine_cases.DEJUMP); every tested difference is recorded and stays a
    factor 2 away from its threshold.
  * RefineOdometry (iOption 0 and 1, with and without ground truth, iStartFrame 0 and 3) and CloseLoopPipeline with the ONE name
    RefinementCore replaced by a scripted stand-in (tests/refine_cases.scripted_core around the reference's own pose algebra).
  * One run with the reference's RefinementCore as written and the registration of RefinePoses.py:295, MyICP.ICP.
The fixture holds data only, written with fixed time stamps: the same arrays give the same bytes.  On another CPU the arrays
themselves differ in their last bits (the inputs come from np.linalg.inv and matrix products, which follow the BLAS kernel chosen for
the CPU); the decisions do not.  The script exits non-zero if caelo.refine disagrees with what the reference computed."""
import ast
import contextlib
import io as _io
import math
import os
import shutil
import sys
import tempfile
import types
import warnings
import zipfile

import numpy as np

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

if not hasattr(np, "bool"):
    np.bool = bool
for n in ("mayavi", "mayavi.mlab"):
    sys.modules[n] = types.ModuleType(n)
sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
cp = types.ModuleType("cupy")   # Voxel.py imports it; nothing here calls it
sys.modules["cupy"] = cp
mpl = types.ModuleType("matplotlib"); mpl.pyplot = types.ModuleType("matplotlib.pyplot")
sys.modules.setdefault("matplotlib", mpl); sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from caelo import refine, stageio, synth  # noqa: E402
import refine_cases as rc                 # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "refine_sequence.npz")
N_FRAMES = (14, 22, 30)
K_PTS = 64          # key points per frame that the inlier files index
N_CLOUD = 400
AXES = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], dtype=np.float64)   # LiDAR -> camera axes


def stub_dirs(base):
    d = types.ModuleType("Dirs")
    d.strBaseDir = base + "/"
    d.strGroundTruthPosesDir = base + "/poses/"
    d.strEstimatedPosesDir = base + "/poses_/"
    d.strDataBaseDir = base + "/velodyne/sequences/"
    d.strCalibDataDir = base + "/calib/"
    sys.modules["Dirs"] = d
    return d


def load_defs(script):
    """The function definitions (and imports) of a reference script, without its module-level code."""
    tree = ast.parse(open(os.path.join(REF, script)).read())
    tree.body = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.FunctionDef))]
    ns = {"__name__": "ref_" + script[:-3]}
    exec(compile(tree, script, "exec"), ns)
    return ns


def quiet(fn, *a, **k):
    buf = _io.StringIO()
    with contextlib.redirect_stdout(buf):
        r = fn(*a, **k)
    return r, buf.getvalue()


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = _io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def hom(pose):
    h = np.eye(4)
    h[:3, :] = np.asarray(pose, np.float64).reshape(3, 4)
    return h


def gt_poses(seq, n):
    out = np.zeros((n, 12))
    for i in range(n):
        (x, y, z), yaw = synth.sensor_pose(40 * seq + i, trajectory="circuit")
        out[i] = np.c_[AXES @ rot("z", math.degrees(yaw)) @ AXES.T, AXES @ np.array([x, y, z])].reshape(12)
    return out


def tr_matrix(rng):
    a = 0.6 * rng.standard_normal(3)
    return np.array(np.c_[AXES @ rot("y", a[1]) @ rot("z", a[2]), [-0.004, -0.076, -0.27]], dtype=np.float32)


def estimate(gt, rng, sigma_deg, sigma_m):
    """The ground truth's relative motions, each followed by a small error, chained from the first pose."""
    out = gt.copy()
    P = hom(gt[0])
    for i in range(1, gt.shape[0]):
        rel = np.linalg.inv(hom(gt[i - 1])) @ hom(gt[i])
        a = sigma_deg * rng.standard_normal(3)
        err = np.eye(4)
        err[:3, :3] = rot("z", a[2]) @ rot("y", a[1]) @ rot("x", a[0])
        err[:3, 3] = sigma_m * rng.standard_normal(3)
        P = P @ rel @ err
        out[i] = P[:3, :].reshape(12)
    return out


def plant(poses, k, deg=0.0, metres=0.0):
    """A jump in the motion into frame k that persists: every pose from k on is carried along."""
    J = np.eye(4)
    J[:3, :3] = rot("y", deg)
    J[:3, 3] = [0.0, 0.0, metres]
    A = hom(poses[k - 1])
    M = A @ J @ np.linalg.inv(A)
    out = poses.copy()
    for j in range(k, poses.shape[0]):
        out[j] = (M @ hom(poses[j]))[:3, :].reshape(12)
    return out


def inlier_files(seq, n, rng):
    """-> per pair (i, i + 1) the arrays (inliersIdx0, inliersIdx1): tracks of key points through consecutive frames."""
    lengths = {0: [1, 1, 3, 3, 5, 5], 1: [1, 1, 3, 3, 3], 2: [1, 1, 3, 3, 25, 25, 25]}[seq]
    perm = [rng.permutation(K_PTS) for _ in range(n)]
    used = [0] * n
    rows = [[] for _ in range(n - 1)]

    def take(f):
        used[f] += 1
        return int(perm[f][used[f] - 1])
    alive = []   # [remaining pairs, index in the current frame]
    for i in range(n - 1):
        for L in lengths:
            if sum(1 for t in alive if t[2] == L) < 2:
                alive.append([L, take(i), L])
        nxt = []
        for t in alive:
            j = take(i + 1)
            rows[i].append((t[1], j))
            if t[0] > 1:
                nxt.append([t[0] - 1, j, t[2]])
        alive = nxt
    out = []
    for i in range(n - 1):
        r = list(rows[i])
        order = rng.permutation(len(r))
        r = [r[o] for o in order]
        if i % 3 == 1:      # a duplicate of an inliersIdx0 entry BEHIND its first occurrence: the first one still counts
            r.append((r[0][0], take(i + 1)))
        if i % 4 == 2:      # ... and IN FRONT of it: the track is diverted to another key point
            r.insert(0, (r[-1][0], take(i + 1)))
        if seq == 1 and i == 10:
            r = []          # an empty pair file
        a = np.array(r, dtype=np.int64).reshape(-1, 2)
        out.append((a[:, 0].copy(), a[:, 1].copy()))
    return out


def static_clouds(gt, Tr, rng):
    """N_CLOUD world points seen from every frame -> [n, N_CLOUD, 3] f32 in each frame's LiDAR coordinates, shuffled per frame."""
    W = AXES @ np.stack([rng.uniform(-20, 32, N_CLOUD), rng.uniform(-25, 25, N_CLOUD), rng.uniform(-2, 5, N_CLOUD)])
    T4 = hom(Tr.astype(np.float64))
    out = []
    for i in range(gt.shape[0]):
        M = np.linalg.inv(hom(gt[i]) @ T4)
        P = (M[:3, :3] @ W + M[:3, 3:4]).T
        out.append(np.array(P[rng.permutation(N_CLOUD)], dtype=np.float32))
    return np.stack(out)


def dejump_decisions(tfm, fwd, poses):
    """FixJumpPoses' loop again around the reference's functions, to record what it compares: -> (fixed, [[dEuler, dT] per frame])."""
    poses_ = poses.copy()
    relRs, relTs, _, dE, dT = tfm["GetDiffRels"](poses_)
    fixed, seen = [], []
    for iFrame in range(2, poses_.shape[0] - 1):
        seen.append([dE[iFrame - 2], dT[iFrame - 2]])
        if dE[iFrame - 2] > 2.0 or dT[iFrame - 2] > 0.5:
            R0, T0 = tfm["GetRtFromOnePose"](poses_[iFrame - 1])
            new = np.c_[np.dot(R0, relRs[iFrame - 2]), np.dot(R0, relTs[iFrame - 2].reshape(3, 1)) + T0].reshape((1, 12))
            poses_, relRs, relTs = fwd(poses_, iFrame, new, relRs, relTs)
            fixed.append(iFrame)
            relRs, relTs, _, dE, dT = tfm["GetDiffRels"](poses_)
    return fixed, np.array(seen)


def differ(bad, what, ours, ref, tol=1e-9):
    ours, ref = np.asarray(ours), np.asarray(ref)
    if ours.shape != ref.shape or (ours.size and not np.abs(ours.astype(np.float64) - ref.astype(np.float64)).max() <= tol):
        bad.append("%s: shapes %s / %s, max |diff| %s" % (what, ours.shape, ref.shape,
                                                          np.abs(ours.astype(np.float64) - ref.astype(np.float64)).max() if ours.shape == ref.shape and ours.size else "-"))


def main():
    rng = np.random.default_rng(20261020)
    tmp = tempfile.mkdtemp(prefix="caelo_refine_")
    base = os.path.join(tmp, "KITTI_odometry")
    D = stub_dirs(base)
    g, bad = {}, []
    try:
        import MyICP as RefICP
        import Transformations
        tfm = vars(Transformations)   # a library module: importing it runs no script
        rp = load_defs("RefinePoses.py")
        ref_core = rp["RefinementCore"]
        ref_fwd = rp["ForwardUpdatePoses"]
        g["n_frames"] = np.array(N_FRAMES, dtype=np.int32)
        gts, ests, trs, inl = [], [], [], []
        for seq, n in enumerate(N_FRAMES):
            ss = "%02d" % seq
            gt = gt_poses(seq, n)
            est = estimate(gt, rng, 0.05, 0.03)
            Tr = tr_matrix(rng)
            files = inlier_files(seq, n, rng)
            gts.append(gt); ests.append(est); trs.append(Tr); inl.append(files)
            seq_dir = D.strDataBaseDir + ss
            for i, (a, b) in enumerate(files):
                stageio.save_inliers(seq_dir, i, i + 1, a, b)
            g["gt_%d" % seq], g["est_%d" % seq], g["tr_%d" % seq] = gt, est, Tr
            g["inl_%d_count" % seq] = np.array([len(a) for a, _ in files], dtype=np.int32)
            g["inl_%d_idx0" % seq] = np.concatenate([a for a, _ in files])
            g["inl_%d_idx1" % seq] = np.concatenate([b for _, b in files])
            g["codes_%d" % seq] = rc.code_table(n)
        clouds = static_clouds(gts[0], trs[0], rng)
        g["clouds_0"] = clouds
        for i in range(N_FRAMES[0]):
            stageio.save_keypts(os.path.join(D.strDataBaseDir + "00", "velodyne", "%06d.bin" % i), clouds[i][:8], ExtendedKeyPts=clouds[i])

        def set_globals(seq, with_gt):
            Tr = trs[seq]
            R_Tr = Tr[:, 0:3]
            R_Tr_inv = np.linalg.inv(R_Tr)
            T_Tr = Tr[:, 3].reshape(3, 1)
            rp.update(PairsDir=os.path.join(D.strDataBaseDir, "%02d" % seq, "InliersIdx") + "/", iGroundTruth=1 if with_gt else 0, R_Tr=R_Tr,
                      R_Tr_inv=R_Tr_inv, T_Tr=T_Tr, T_Tr_inv=-np.dot(R_Tr_inv, T_Tr), iShowMatchingResult=0, strDataBaseDir=D.strDataBaseDir)

        def pairs_of(seq):
            return lambda f0, f1: inl[seq][f0]

        # ---- GetTransferPairIdx on its own: duplicates, no common value, empty inputs --------------------------------------------------
        tp = [(np.array([3, 5, 5, 9, 11]), np.array([5, 3, 3, 7, 11, 5])), (np.array([1, 2]), np.array([3, 4])), (np.array([], dtype=np.int64), np.array([1])),
              (np.array([4]), np.array([], dtype=np.int64)), (inl[2][4][1], inl[2][5][0])]
        for k, (a, b) in enumerate(tp):
            ref = np.array(rp["GetTransferPairIdx"](a, b), dtype=np.int64).reshape(-1, 2)
            ours = np.array(refine.GetTransferPairIdx(a, b), dtype=np.int64).reshape(-1, 2)
            if not np.array_equal(ref, ours):
                bad.append("GetTransferPairIdx %d" % k)
            g["transfer_%d_a" % k], g["transfer_%d_b" % k], g["transfer_%d_out" % k] = a, b, ref
        g["transfer_n"] = np.array(len(tp))

        # ---- GetDiffRels and FixJumpPoses ---------------------------------------------------------------------------------------------
        n0 = N_FRAMES[0]
        planted = {"rotation": plant(ests[0], 6, deg=6.0), "translation": plant(ests[0], 7, metres=1.5), "both": plant(ests[0], 5, deg=-7.0, metres=-1.4),
                   "frame_2": plant(ests[0], 2, deg=6.5), "frame_n_2": plant(ests[0], n0 - 2, metres=1.6),
                   "two_in_a_row": plant(plant(ests[0], 8, deg=6.0, metres=1.2), 9, deg=-8.0), "none": ests[0]}
        assert tuple(planted) == rc.DEJUMP
        for name, poses in planted.items():
            out, log = quiet(rp["FixJumpPoses"], poses)
            fixed_ref = ast.literal_eval(log.strip().splitlines()[-1])
            fixed, seen = dejump_decisions(tfm, ref_fwd, poses)
            assert fixed == fixed_ref, (name, fixed, fixed_ref)
            flagged = (seen[:, 0] > 2.0) | (seen[:, 1] > 0.5)
            clear = ((seen[:, 0] > 4.0) | (seen[:, 1] > 1.0)) | ((seen[:, 0] < 1.0) & (seen[:, 1] < 0.25))
            assert clear.all() and flagged.sum() == len(fixed), (name, seen)
            ours, ofixed = refine.FixJumpPoses(poses)
            if ofixed != fixed_ref:
                bad.append("FixJumpPoses %s: %s vs %s" % (name, ofixed, fixed_ref))
            differ(bad, "FixJumpPoses %s poses" % name, ours, out)
            g["dejump_%s_in" % name], g["dejump_%s_out" % name] = poses, np.asarray(out)
            g["dejump_%s_fixed" % name], g["dejump_%s_seen" % name] = np.array(fixed_ref, dtype=np.int32), seen
            print("  FixJumpPoses %-13s fixed %s" % (name, fixed_ref))
        for k, ours in enumerate(refine.GetDiffRels(planted["both"])):
            differ(bad, "GetDiffRels %d" % k, ours, tfm["GetDiffRels"](planted["both"])[k], tol=1e-12)
        for k, name in enumerate(("relRs", "relTs", "relEulers", "diffEulers", "diffTs")):
            g["diffrels_" + name] = tfm["GetDiffRels"](planted["both"])[k]

        # ---- RefineOdometry and CloseLoopPipeline around the scripted stand-in ------------------------------------------------------------
        def reference_walk(seq, iOption, with_gt, start, core7):
            """-> (poses___, aDebugInfo, failed, poses____): the reference's two functions with RefinementCore = core7."""
            set_globals(seq, with_gt)
            rp["RefinementCore"] = core7
            debug = [gts[seq]] if with_gt else []
            (poses3, info), log = quiet(rp["RefineOdometry"], "%02d" % seq, ests[seq], trs[seq], iOption=iOption, debugInfo=debug, iStartFrame=start)
            failed = ast.literal_eval(log.strip().splitlines()[-1])
            return poses3, info, failed

        for name, (seq, iOption, with_gt, start) in rc.WALKS.items():
            calls = []
            core = rc.scripted_core(g["codes_%d" % seq], gts[seq], ref_fwd, tfm["GetRelRtBetween2Poses"], tfm["GetRtFromOnePose"], calls)
            core7 = lambda poses, strSequence, f0, f1, relRs, relTs, thr: core(poses, f0, f1, relRs, relTs, thr)   # noqa: E731
            poses3, info, failed = reference_walk(seq, iOption, with_gt, start, core7)
            tried = [(a, b, int(g["codes_%d" % seq][a, b])) for a, b, _ in calls]
            assert all(t == 1.0 for _, _, t in calls)
            n_first = len(calls)
            if info.ndim == 2 and info.shape[0] >= 3:
                (poses4, _), _ = quiet(rp["CloseLoopPipeline"], "%02d" % seq, poses3, trs[seq], info)
            else:
                poses4 = poses3
            second = [(a, b, int(g["codes_%d" % seq][a, b])) for a, b, _ in calls[n_first:]]
            assert all(t == 0.5 for _, _, t in calls[n_first:])
            ocalls = []
            ocore = rc.scripted_core(g["codes_%d" % seq], gts[seq], refine.ForwardUpdatePoses, refine.GetRelRtBetween2Poses, refine.GetRtFromOnePose, ocalls)
            o3, oinfo, ofailed, otried = refine.RefineOdometry(ests[seq], iOption, ocore, pairs=pairs_of(seq), gt=gts[seq] if with_gt else None, iStartFrame=start)
            o4, osecond = refine.CloseLoopPipeline(o3, oinfo, ocore)
            if otried != tried or [list(map(int, f)) for f in ofailed] != [list(map(int, f)) for f in failed] or osecond != second:
                bad.append("walk %s: decisions differ\n   %s\n   %s" % (name, otried, tried))
            differ(bad, "walk %s poses" % name, o3, poses3)
            differ(bad, "walk %s debug" % name, oinfo, info, tol=1e-5)
            differ(bad, "walk %s second pass" % name, o4, poses4)
            g["walk_%s_tried" % name] = np.array(tried, dtype=np.int32).reshape(-1, 3)
            g["walk_%s_failed" % name] = np.array(failed, dtype=np.int32).reshape(-1, 2)
            g["walk_%s_poses" % name], g["walk_%s_debug" % name] = np.asarray(poses3), info
            g["walk_%s_second" % name] = np.array(second, dtype=np.int32).reshape(-1, 3)
            g["walk_%s_second_poses" % name] = np.asarray(poses4)
            print("  walk %-17s %2d calls, codes %s, spans up to %d, failed %s, debug %s, second pass %d calls"
                  % (name, len(tried), sorted({c for _, _, c in tried}), max(b - a for a, b, _ in tried), failed, info.shape, len(second)))
        for name in rc.WALKS:
            print("   ", name, g["walk_%s_tried" % name].tolist())
        kinds = {(min(b - a, 2), c) for name in ("keyframes_gt", "keyframes_nogt") for a, b, c in g["walk_%s_tried" % name].tolist()}
        assert kinds == {(s, c) for s in (1, 2) for c in (-1, 0, 1)}, kinds   # every code on long and on one-frame pairs
        assert max(b - a for a, b, _ in g["walk_keyframes_gt_tried"].tolist()) == 20   # a chain that outlives nMaxTransferFrames
        assert len(g["walk_consecutive_nogt_second"]) >= 2

        # ---- the reference's RefinementCore as written, with the registration of :295 -----------------------------------------------------
        seq = 0
        set_globals(seq, True)
        rp["RefinementCore"] = ref_core
        icp_out, core_calls, margins = [], [], []

        def icp_295(KeyPts0, KeyPts1_, PlanarPts0, PlanarPts1_, **kw):
            R, T, ok = RefICP.ICP(KeyPts0, KeyPts1_)
            icp_out.append((np.array(R), np.array(T).reshape(3), bool(ok)))
            return R, T, ok

        def recording_core(poses, strSequence, f0, f1, relRs, relTs, thr):
            r = ref_core(poses, strSequence, f0, f1, relRs, relTs, thr)
            core_calls.append((int(f0), int(f1), int(r[0])))
            # what :304-309 compared, from the registration's result: recorded so that the test can assert its distance to 10 deg / 5 m
            oR, oT = tfm["GetLidarRelRtBetween2Poses"](poses[f0, :], poses[f1, :], rp["R_Tr"], rp["T_Tr"], rp["R_Tr_inv"], rp["T_Tr_inv"])
            R, T, _ = icp_out[-1]
            nR, nT = np.dot(R, oR), np.dot(R, oT) + T.reshape(3, 1)
            margins.append([np.linalg.norm(tfm["RotateMat2EulerAngle_XYZ"](oR) - tfm["RotateMat2EulerAngle_XYZ"](nR)), np.linalg.norm(oT - nT)])
            return r
        rp["ICP_Pt2PtAndPt2Plane"] = icp_295
        rp["RefinementCore"] = recording_core
        (poses3, info), log = quiet(rp["RefineOdometry"], "00", ests[0], trs[0], iOption=1, debugInfo=[gts[0]], iStartFrame=0)
        failed = ast.literal_eval(log.strip().splitlines()[-1])
        n_first = len(core_calls)
        (poses4, _), _ = quiet(rp["CloseLoopPipeline"], "00", poses3, trs[0], info)
        assert all(ok for _, _, ok in icp_out) and all(c == 1 for _, _, c in core_calls), core_calls
        okeypts = lambda f: (clouds[f], np.zeros((0, 6), np.float32))   # noqa: E731
        ocore = refine.make_core(okeypts, trs[0], refine.pt2pt_adapter(lambda a, b: quiet(RefICP.ICP, a, b)[0]))
        o3, oinfo, ofailed, otried = refine.RefineOdometry(ests[0], 1, ocore, pairs=pairs_of(0), gt=gts[0], iStartFrame=0)
        o4, osecond = refine.CloseLoopPipeline(o3, oinfo, ocore)
        if otried != core_calls[:n_first] or osecond != core_calls[n_first:] or ofailed != failed:
            bad.append("real ICP walk: decisions differ\n   %s\n   %s" % (otried + osecond, core_calls))
        differ(bad, "real ICP walk poses", o3, poses3)
        differ(bad, "real ICP walk debug", oinfo, info, tol=1e-5)
        differ(bad, "real ICP second pass", o4, poses4)
        g["real_tried"] = np.array(core_calls[:n_first], dtype=np.int32).reshape(-1, 3)
        g["real_second"] = np.array(core_calls[n_first:], dtype=np.int32).reshape(-1, 3)
        g["real_failed"] = np.array(failed, dtype=np.int32).reshape(-1, 2)
        g["real_poses"], g["real_debug"], g["real_second_poses"] = np.asarray(poses3), info, np.asarray(poses4)
        g["real_margins"] = np.array(margins)
        assert (g["real_margins"][:, 0] < 5.0).all() and (g["real_margins"][:, 1] < 2.5).all(), margins
        print("  real ICP walk: pairs %s, second pass %s, RTE %.4f -> %.4f (mean)" % ([(a, b) for a, b, _ in core_calls[:n_first]],
              [(a, b) for a, b, _ in core_calls[n_first:]], info[:, 4].mean(), info[:, 6].mean()))
        assert info[:, 6].mean() < 0.5 * info[:, 4].mean()   # the refinement does refine
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for b in bad:
        print("MISMATCH", b)
    save_npz(OUT, g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
