#!/opt/conda/bin/python3.9
"""Generate tests/golden/evaluate.npz from the reference's evaluation scripts (read-only reference tree, see make_goldens.py).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tools/make_goldens_evaluate.py

Interpreter: the conda python3.9 (NumPy 1.26, scikit-learn 0.24.2), like tools/make_goldens.py.  A small KITTI-shaped tree is
written to a temporary directory: 11 sequences of 18-24 frames, ground truth on synth.sensor_pose(trajectory="circuit"), perturbed
estimates for every method the scripts loop over, a non-identity Tr per sequence, key point files for the three sources (K from 4
to 1500, duplicated coordinates, a stop of the vehicle that repeats a whole frame), and matchability files written by
caelo.evaluate.save_matchability.

The reference runs two ways:
  * its functions (TranslatePtsIntoWorldFrame, GetAllKeyPts, GetPairDistances, ComputeDispersionOfKeypoints, GetErrorRTs), the
    definitions loaded from the script files at run time;
  * the aggregation scripts as written (EvaluationOnRegistration.py, EvalOnReg_KeyPts.py, EvaluationOnKeypts.py) through a stub
    ``Dirs`` module that points into the temporary tree, so that their module-level loops write their own .mat files.  Only the
    loop constants the scripts keep as plain assignments (frame steps, sources, mode) are set per run.
The fixture holds data only.  The script exits non-zero if caelo.evaluate's host code disagrees with what the reference computed.
"""
import ast
import math
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

if not hasattr(np, "bool"):
    np.bool = bool
if not hasattr(np, "int"):
    np.int = int   # EvalOnReg_KeyPts.py:186,197-198
for n in ("mayavi", "mayavi.mlab"):
    sys.modules[n] = types.ModuleType(n)
sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
mpl = types.ModuleType("matplotlib"); mpl.pyplot = types.ModuleType("matplotlib.pyplot")
sys.modules.setdefault("matplotlib", mpl); sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

from scipy import io  # noqa: E402
from sklearn.neighbors import NearestNeighbors  # noqa: E402

from caelo import evaluate as ev, keysources, synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "evaluate.npz")
N_SEQ = 11
SOURCES = ("ae", "3dfeatnet", "usip")
STEPS = (1, 2, 10)
REG_METHODS = [(k, d) for k in range(3) for d in range(3)] + [(k, 2) for k in range(3, 6)]   # EvaluationOnRegistration + EvalOnReg_KeyPts


def stub_dirs(base):
    """The names the scripts take from ``from Dirs import *``, pointing into ``base`` (trailing separators: the scripts concatenate)."""
    d = types.ModuleType("Dirs")
    d.strBaseDir = base + "/"
    d.strGroundTruthPosesDir = base + "/poses/"
    d.strEstimatedPosesDir = base + "/poses_"
    d.strDataBaseDir = base + "/velodyne/sequences/"
    d.strCalibDataDir = base + "/calib/"
    d.str3DFeatNetDir = base + "/3dfeatnet/"
    d.strUsipKeyPtsDir = base + "/usip/"
    sys.modules["Dirs"] = d
    return d


def load_defs(script):
    """The function definitions (and imports) of a reference script, without its module-level loops."""
    tree = ast.parse(open(os.path.join(REF, script)).read())
    tree.body = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.FunctionDef))]
    ns = {"__name__": "ref_" + script[:-3]}
    exec(compile(tree, script, "exec"), ns)
    return ns


def run_script(script, cwd, **consts):
    """Run a reference script as written; ``consts`` replaces the value of a top-level ``name = <literal>`` assignment and
    ``ranges`` the bounds of the source loop (``range(2,3,1)`` of EvaluationOnKeypts.py)."""
    tree = ast.parse(open(os.path.join(REF, script)).read())
    ranges = consts.pop("ranges", None)
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in consts:
            node.value = ast.parse(repr(consts[node.targets[0].id]), mode="eval").body
        if ranges is not None and isinstance(node, ast.For) and isinstance(node.target, ast.Name) and node.target.id == "iDataSource":
            node.iter = ast.parse("range(%d, %d, 1)" % ranges, mode="eval").body
    ast.fix_missing_locations(tree)
    old = os.getcwd()
    os.chdir(cwd)
    try:
        import contextlib
        import io as _io
        with contextlib.redirect_stdout(_io.StringIO()):
            exec(compile(tree, script, "exec"), {"__name__": "__main__"})
    finally:
        os.chdir(old)


def gt_poses(seq, n):
    """KITTI-style camera poses [n, 12] of the circuit trajectory (camera axes: x right, y down, z forward; the LiDAR's x forward)."""
    C = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], dtype=np.float64)   # LiDAR -> camera axes
    out = np.zeros((n, 12))
    for i in range(n):
        (x, y, z), yaw = synth.sensor_pose(40 * seq + i, trajectory="circuit")
        if seq == 1 and i == 5:   # a stop: frame 5 where frame 4 was (whole frames repeat in the world)
            (x, y, z), yaw = synth.sensor_pose(40 * seq + 4, trajectory="circuit")
        c, s = math.cos(yaw), math.sin(yaw)
        R = C @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ C.T
        T = C @ np.array([x, y, z])
        out[i] = np.c_[R, T].reshape(12)
    return out


def tr_matrix(seq, rng):
    a = 0.01 * rng.standard_normal(3)
    Rz = np.array([[math.cos(a[2]), -math.sin(a[2]), 0], [math.sin(a[2]), math.cos(a[2]), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(a[1]), 0, math.sin(a[1])], [0, 1, 0], [-math.sin(a[1]), 0, math.cos(a[1])]])
    C = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], dtype=np.float64)
    Tr = np.c_[C @ Ry @ Rz, [-0.004, -0.076, -0.27]]
    return np.array(Tr, dtype=np.float32)


def perturb(poses, k, d, rng):
    """An estimate: the ground truth with a chained per-frame error that grows with the method index (some pairs fail)."""
    out = poses.copy()
    drift = np.eye(4)
    for i in range(1, poses.shape[0]):
        sc = 0.02 * (1 + k + d)
        if rng.random() < 0.08 * (k + 1):
            sc *= 40   # a failed pair
        a = np.radians(sc) * rng.standard_normal(3)
        cx, sx, cy, sy, cz, sz = math.cos(a[0]), math.sin(a[0]), math.cos(a[1]), math.sin(a[1]), math.cos(a[2]), math.sin(a[2])
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        step = np.eye(4); step[:3, :3] = R; step[:3, 3] = 0.5 * sc * rng.standard_normal(3)
        drift = drift @ step
        P = np.eye(4); P[:3, :] = poses[i].reshape(3, 4)
        out[i] = (P @ drift)[:3, :].reshape(12)
    return np.array(out, dtype=np.float32)   # pose files of the engine hold float32 rows


def keypoint_counts(seq, n, rng):
    k = rng.integers(6, 28, size=n)
    if seq == 0:
        k[2], k[3], k[6], k[7] = 4, 5, 1500, 1100   # the smallest kd-tree sets; more than one LDS chunk (csrc/evaluate.hip)
    return k


def raw_keypoints(k, rng, prev=None):
    pts = np.c_[rng.uniform(-40, 40, k), rng.uniform(-40, 40, k), rng.uniform(-2, 3, k)].astype(np.float32)
    if k > 8:
        pts[k // 2] = pts[1]            # a coordinate that repeats inside the set
        pts[k - 1, 0] = pts[0, 0]       # and a repeated x
    if prev is not None and k > 6:
        m = min(k, prev.shape[0]) // 3
        pts[:m] = prev[:m]              # points seen again (nearly the same world points one frame on)
    return pts


def boundary_sets():
    """World-frame sets with query points at exactly D, just below and just above every threshold from a fit point at the origin."""
    fit = np.array([[0, 0, 0], [100, 0, 0], [0, 100, 0], [0, 0, 100], [100, 100, 100]], dtype=np.float64)
    q = []
    for D in ev.DISCRETIZATIONS:
        for x in (np.nextafter(D, 0.0), D, np.nextafter(D, np.inf)):
            q.append([x, 0.0, 0.0])
            q.append([0.0, -x, 0.0])
    return fit, np.array(q, dtype=np.float64)


def sk_nn(fit, query):
    nbrs = NearestNeighbors(n_neighbors=1, algorithm="auto").fit(fit)
    assert nbrs._fit_method == "kd_tree", nbrs._fit_method
    return nbrs.kneighbors(query)[0]


def main():
    rng = np.random.default_rng(20261016)
    tmp = tempfile.mkdtemp(prefix="caelo_eval_")
    base = os.path.join(tmp, "KITTI_odometry")
    D = stub_dirs(base)
    g = {}
    bad = []
    try:
        nfr = np.array([24 if s == 0 else int(rng.integers(18, 25)) for s in range(N_SEQ)], dtype=np.int32)
        g["n_frames"] = nfr
        gts, trs, ests, kps, kcounts, match = [], [], [], {s: [] for s in SOURCES}, {s: [] for s in SOURCES}, []
        for seq in range(N_SEQ):
            ss = "%02d" % seq
            n = int(nfr[seq])
            gt = gt_poses(seq, n)
            gts.append(gt)
            os.makedirs(D.strGroundTruthPosesDir, exist_ok=True)
            np.savetxt(D.strGroundTruthPosesDir + ss + ".txt", gt)
            Tr = tr_matrix(seq, rng)
            trs.append(Tr)
            os.makedirs(D.strCalibDataDir + ss, exist_ok=True)
            calib = np.zeros((5, 12)); calib[:4] = np.eye(3, 4).reshape(12); calib[4] = Tr.astype(np.float64).reshape(12)
            np.savetxt(D.strCalibDataDir + ss + "/calib_.txt", calib, fmt="%.17g")
            for (k, d) in REG_METHODS:
                est = perturb(gt, k, d, rng)
                ests.append(est)
                for step in STEPS:
                    os.makedirs(D.strEstimatedPosesDir, exist_ok=True)
                    np.savetxt(os.path.join(D.strEstimatedPosesDir, "%d_%d-%d_%s.txt" % (step, k, d, ss)), est)
                ni = rng.integers(0, 400, size=n - 1); npairs = ni + rng.integers(1, 600, size=n - 1); it = rng.integers(1, 120, size=n - 1)
                match.append(np.stack([ni, npairs, it]).astype(np.int16))
                for step in STEPS:
                    ev.save_matchability(os.path.join(D.strBaseDir, "Matchablity_%d_%d-%d_%s.mat" % (step, k, d, ss)), ni, npairs, it)
            counts = keypoint_counts(seq, n, rng)
            for src in SOURCES:
                prev = None
                for i in range(n):
                    pts = raw_keypoints(int(counts[i]), rng, prev)
                    if seq == 1 and i == 5:
                        pts = kps[src][-1].copy()   # the stop: the same scan's key points again
                    prev = pts
                    kps[src].append(pts)
                    kcounts[src].append(pts.shape[0])
                    if src == "ae":
                        p = os.path.join(D.strDataBaseDir + ss, "KeyPts", "%06d.bin.mat" % i)
                        os.makedirs(os.path.dirname(p), exist_ok=True)
                        io.savemat(p, {"KeyPts": pts})
                    elif src == "3dfeatnet":
                        keysources.write_3dfeatnet(D.str3DFeatNetDir + "Descriptors/" + ss + "/%06d.bin" % i, pts)
                    else:
                        keysources.write_usip(D.strUsipKeyPtsDir + ss + "/%06d.bin" % i, pts)
        g["gt_poses"] = np.concatenate(gts)
        g["tr"] = np.stack(trs)
        g["est_poses"] = np.stack([np.concatenate(ests[m::len(REG_METHODS)]) for m in range(len(REG_METHODS))])   # [method, rows, 12] f32
        g["reg_methods"] = np.array(REG_METHODS, dtype=np.int32)
        g["matchability"] = np.stack([np.concatenate(match[m::len(REG_METHODS)], axis=1) for m in range(len(REG_METHODS))])   # [method, 3, pairs]
        for src in SOURCES:
            g["kp_" + src] = np.concatenate(kps[src])
            g["kp_count_" + src] = np.array(kcounts[src], dtype=np.int32)

        # ---- the reference's functions -------------------------------------------------------------------------------------
        ekp = load_defs("EvaluationOnKeypts.py")
        tfm = load_defs("Transformations.py")
        vis = load_defs("Visualization.py")
        ref_dists = {}
        for si, src in enumerate(SOURCES):
            for step in STEPS:
                world_all, d0_all, d1_all, n_world = [], [], [], []
                for seq in range(N_SEQ):
                    ss = "%02d" % seq
                    ref_list = ekp["GetAllKeyPts"](ss, step, si)
                    kp_dir = {"ae": D.strDataBaseDir + ss + "/KeyPts", "3dfeatnet": D.str3DFeatNetDir + "Descriptors/" + ss,
                              "usip": D.strUsipKeyPtsDir + ss}[src]
                    ours = ev.GetAllKeyPts(D.strDataBaseDir + ss + "/KeyPts" if src == "ae" else kp_dir, src, gts[seq], trs[seq], step)
                    if len(ours) != len(ref_list) or any(a.dtype != b.dtype or not np.array_equal(a, b) for a, b in zip(ours, ref_list)):
                        bad.append("GetAllKeyPts %s seq %s step %d" % (src, ss, step))
                    d0 = ekp["GetPairDistances"](ref_list)
                    d1 = ekp["ComputeDispersionOfKeypoints"](ref_list)
                    for a, b in ((ref_list[0], ref_list[1]),):
                        assert np.array_equal(sk_nn(a, b), d0[:b.shape[0]])
                    if step == 1:
                        world_all += ref_list
                    n_world.append(len(ref_list))
                    d0_all.append(d0.ravel()); d1_all.append(d1.ravel())
                    ref_dists[(0, step, si, seq)], ref_dists[(1, step, si, seq)] = d0, d1
                if step == 1:
                    g["world_%s" % src] = np.concatenate(world_all)
                    if src == "usip":
                        assert g["world_usip"].dtype == np.float64
                    else:
                        assert g["world_%s" % src].dtype == np.float32
                g["dist0_%s_%d" % (src, step)] = np.concatenate(d0_all)
                g["dist1_%s_%d" % (src, step)] = np.concatenate(d1_all)
                assert not g["dist1_%s_%d" % (src, step)].any()   # mode 1: every distance is 0 (EvaluationOnKeypts.py:93)

        # the world-frame round trip through the reference's TranslatePtsIntoWorldFrame, both dtype paths
        pose = np.array(gts[3][2].reshape(3, 4), dtype=np.float32)
        for pts in (kps["ae"][5], np.dot(keysources.R90, kps["usip"][5].T).T):
            a, b = ev.TranslatePtsIntoWorldFrame(pose, trs[3], pts), tfm["TranslatePtsIntoWorldFrame"](pose, trs[3], pts)
            if a.dtype != b.dtype or not np.array_equal(a, b):
                bad.append("TranslatePtsIntoWorldFrame %s" % b.dtype)

        # boundary sets: distances exactly at, below and above every threshold
        fit, q = boundary_sets()
        g["boundary_fit"], g["boundary_query"] = fit, q
        g["boundary_dist"] = sk_nn(fit, q).ravel()
        g["boundary_counts"] = np.array(ev.RepeatabilityCounts(g["boundary_dist"].reshape(-1, 1)), dtype=np.int64)   # (the host loop, pinned below)

        # GetErrorRTs of every method, sequence and step
        errs_e, errs_t = [], []
        for m, (k, d) in enumerate(REG_METHODS):
            for step in STEPS:
                for seq in range(N_SEQ):
                    gt = np.loadtxt(D.strGroundTruthPosesDir + "%02d.txt" % seq)
                    est = np.loadtxt(os.path.join(D.strEstimatedPosesDir, "%d_%d-%d_%02d.txt" % (step, k, d, seq)))
                    n = gt.shape[0]
                    Tr = np.array(np.loadtxt(D.strCalibDataDir + "%02d/calib_.txt" % seq)[4, :].reshape(3, 4), dtype=np.float32)
                    _, _, re, rt = vis["GetErrorRTs"](gt[0:n:step, :], est[0:n:step, :], Tr, isPlot=0)
                    _, _, oe, ot = ev.GetErrorRTs(gt, est, ev.read_tr(D.strCalibDataDir + "%02d/calib_.txt" % seq), step)
                    if re.dtype != oe.dtype or rt.dtype != ot.dtype or not (np.array_equal(re, oe) and np.array_equal(rt, ot)):
                        bad.append("GetErrorRTs method %s step %d seq %d (max |diff| %.3g / %.3g)" % ((k, d), step, seq, np.abs(re - oe).max(), np.abs(rt - ot).max()))
                    if m == 0 or step == 1:
                        errs_e.append(re); errs_t.append(rt)
        g["err_eulers"] = np.concatenate(errs_e)   # method 0 at steps 1, 2, 10, then methods 1.. at step 1 (sequence order inside)
        g["err_ts"] = np.concatenate(errs_t)

        # ---- the aggregation scripts as written ------------------------------------------------------------------------------
        run_script("EvaluationOnRegistration.py", tmp)
        g["EvaluationResults"] = io.loadmat(os.path.join(D.strBaseDir, "EvaluationResults.mat"))["EvaluationResults"]
        for step in STEPS:
            run_script("EvalOnReg_KeyPts.py", tmp, iFrameStep=step)
            g["EvaluationResults_KeyPts_%d" % step] = io.loadmat(os.path.join(D.strBaseDir, "EvaluationResults-KeyPts.mat"))["EvaluationResults"]
        for mode in (0, 1):
            run_script("EvaluationOnKeypts.py", tmp, mode=mode, iFrameSteps=list(STEPS), ranges=(0, 3))
        files = {}
        for mode, title in ((0, "AccuracyOfKeyPts_"), (1, "InnerAccuracyOfKeyPts_")):
            for step in STEPS:
                for si in range(3):
                    for seq in range(N_SEQ):
                        c = io.loadmat(os.path.join(D.strBaseDir, "%s%d_%d_%02d.mat" % (title, step, si, seq)))["counts"]
                        files[(mode, step, si, seq)] = c
                        ours = ev.RepeatabilityCounts(ref_dists[(mode, step, si, seq)])
                        if c.shape != (1, len(ours)) or c.ravel().tolist() != [int(x) for x in ours]:
                            bad.append("RepeatabilityCounts mode %d step %d source %d seq %d" % (mode, step, si, seq))
        g["counts_shape"] = np.array(files[(0, 1, 0, 0)].shape)
        g["counts_dtype"] = np.array(str(files[(0, 1, 0, 0)].dtype))
        g["counts"] = np.stack([np.stack([np.stack([np.stack([files[(mode, step, si, seq)].ravel() for seq in range(N_SEQ)])
                                                    for si in range(3)]) for step in STEPS]) for mode in (0, 1)])   # [mode, step, source, seq, T+1]

        # our rows against the scripts'
        for step, key in [(1, "EvaluationResults")] + [(s, "EvaluationResults_KeyPts_%d" % s) for s in STEPS]:
            methods = [(k, d) for k in range(3) for d in range(3)] if key == "EvaluationResults" else [(k, 2) for k in range(6)]
            for (k, d) in methods:
                seqs = []
                for seq in range(N_SEQ):
                    gt = np.loadtxt(D.strGroundTruthPosesDir + "%02d.txt" % seq)
                    est = np.loadtxt(os.path.join(D.strEstimatedPosesDir, "%d_%d-%d_%02d.txt" % (step, k, d, seq)))
                    _, _, e, t = ev.GetErrorRTs(gt, est, ev.read_tr(D.strCalibDataDir + "%02d/calib_.txt" % seq), step)
                    prop, trials = ev.load_matchability(os.path.join(D.strBaseDir, "Matchablity_%d_%d-%d_%02d.mat" % (step, k, d, seq)))
                    seqs.append((e, t, prop, trials))
                row, ok = ev.RegistrationRow(seqs)
                ref = g[key][k * 3 + d]
                if key != "EvaluationResults":   # EvalOnReg_KeyPts.py:165,168 report percentages
                    row[4] = 100 * np.sum(ok) / ok.shape[0]
                    row[5] = 100 * row[5]
                if not np.array_equal(row, ref):
                    bad.append("RegistrationRow %s %s: %s vs %s" % (key, (k, d), row, ref))
        g["success_rate_col"] = g["EvaluationResults"][:, 4]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for b in bad:
        print("MISMATCH", b)
    np.savez_compressed(OUT, **g)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    return 1 if bad else 0



if __name__ == "__main__":
    sys.exit(main())
