#!/opt/conda/bin/python3.9
"""Generate tests/golden/keysources.npz by IMPORTING THE REFERENCE: the key point sources other than the detector
(PoseEstimation.py:26-45, iKeyPtSource 1 = 3DFeatNet, 2 = USIP).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tools/make_goldens_keysources.py

Same interpreter, stubs and division of labour as tools/make_goldens.py (that file is left as it is): the reference's own
EulerAngle2RotateMat, the R90 product of PoseEstimation.py:39, GetPatchesList and SolveRelativePose (NumPy's global generator
seeded per pair); the voxel lists come from the oracle's Voxelization and the encoder's ``predict`` from the oracle's restatement,
both pinned to the reference by tools/make_goldens.py.

Synthetic key point files: per frame of two consecutive synthetic scans, 400 scan points with seeded noise -- written in USIP's axes
(R90^T applied, float32) for source 2, and as the xyz columns of a [-1, 35] 3DFeatNet record for source 1 -- plus, for source 1,
points beyond every face of the voxel grid (negative side included), far away, and duplicated.

USIP precision: the reference keeps the rotated points in float64; the engine rounds them to float32.  The script runs the
reference both ways and prints (and stores) how many key voxels, patches and poses the float64 run would change.  The golden's
patches / poses are those of the float32 points (what the engine is compared with).
"""
import contextlib
import io
import math
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

if not hasattr(np, "bool"):
    np.bool = bool  # Match.py:179,193
for n in ("mayavi", "mayavi.mlab"):
    sys.modules[n] = types.ModuleType(n)
sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
cp = types.ModuleType("cupy")  # every CuPy symbol used in SphericalRing.py:137-206 (imported by Match.py; not called here)
for k in ("array", "zeros", "min", "sum", "squeeze", "int32", "float32"):
    setattr(cp, k, getattr(np, k))
cp.bool = bool
cp.asnumpy = np.asarray
cp.argsort = lambda a: np.argsort(a, kind="stable")
sys.modules["cupy"] = cp
mpl = types.ModuleType("matplotlib"); mpl.pyplot = types.ModuleType("matplotlib.pyplot")
sys.modules.setdefault("matplotlib", mpl); sys.modules.setdefault("matplotlib.pyplot", mpl.pyplot)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

import warnings
warnings.filterwarnings("ignore")
import Transformations as RefTf  # noqa: E402
import Voxel as RefVoxel         # noqa: E402
import Match as RefMatch         # noqa: E402

import oracle as orc             # noqa: E402
from caelo import synth          # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "keysources.npz")
FRAMES = (4, 5)
SEED_BASE = 300


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def key_voxels(pts):
    off = np.array([RefVoxel.VisibleLength, RefVoxel.VisibleWidth, RefVoxel.VisibleHeight])
    return [np.array((pts + off) / RefVoxel.VoxelSizes[s], dtype=np.int32) for s in range(3)]   # Voxel.py:185,:193


def main():
    _, enc = orc.load_models(os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5"),
                             os.path.join(REPO, "weights", "EncoderModel4VoxelPatch.h5"))
    R90 = RefTf.EulerAngle2RotateMat(-math.pi / 2, 0, -math.pi / 2, "xyz")   # PoseEstimation.py:177
    g = {"r90_bits": R90.view(np.uint64).copy(), "frames": np.array(FRAMES), "seed_base": SEED_BASE}
    grid = (RefVoxel.VisibleLength, RefVoxel.VisibleWidth, RefVoxel.VisibleHeight)
    per = {}
    for f in FRAMES:
        pc = synth.make_scan(f)
        g["cloud_sha256_%d" % f] = synth.cloud_sha256(pc)
        vox = orc.Voxelization(pc[:, 0:3])[6:9]
        rs = np.random.RandomState(1000 + f)
        on = pc[rs.choice(pc.shape[0], 400, replace=False), 0:3].astype(np.float64) + rs.normal(0, 0.05, (400, 3))
        usip_raw = np.ascontiguousarray(np.dot(R90.T, on.T).T, dtype=np.float32)          # what a USIP file holds (its own axes)
        rot64 = np.dot(R90, usip_raw.T).T                                                  # PoseEstimation.py:39, float64
        rot32 = rot64.astype(np.float32)
        off = []
        for a in range(3):                                                                 # beyond each face, both sides
            for sgn in (-1.0, 1.0):
                p = np.zeros(3); p[a] = sgn * (grid[a] + 1.5); off.append(p)
                q = np.zeros(3); q[a] = sgn * (grid[a] + 40.0); off.append(q)
        off += [np.array([-10000.0, 5.0, 0.0]), np.array([9000.0, -9000.0, 900.0])]
        feat_pts = np.concatenate([on[:300], np.array(off), on[:4]]).astype(np.float32)   # + four duplicates
        g["usip_raw_%d" % f], g["usip_rot64_%d" % f], g["usip_rot32_%d" % f] = usip_raw, rot64, rot32
        g["featnet_pts_%d" % f] = feat_pts
        for name, pts in (("usip", rot32), ("usip64", rot64), ("featnet", feat_pts)):
            _, plist = quiet(RefVoxel.GetPatchesList, pts, *vox)
            bits = np.stack([orc.pack_patches(plist[s]) for s in range(3)], axis=1)        # [K, 3, 64]
            feats = np.c_[tuple(enc.predict(plist[s]) for s in range(3))]                  # GetFeaturesFromPatches (Match.py:130-135)
            per[(name, f)] = (pts, bits, feats)
            if name != "usip64":
                g["%s_bits_%d" % (name, f)] = bits
                g["%s_features_%d" % (name, f)] = feats
    f0, f1 = FRAMES
    counts = {}
    for name in ("usip", "usip64", "featnet"):
        p0, _, F0 = per[(name, f0)]
        p1, _, F1 = per[(name, f1)]
        np.random.seed(SEED_BASE + f0)        # pair (f0, f1): RandomState(seed) is the stream of engine.ransac_draws(seed)
        W0, W1 = np.ones((p0.shape[0], 1), np.float32), np.ones((p1.shape[0], 1), np.float32)
        R, T, ok, i0, i1, thr = quiet(RefMatch.SolveRelativePose, p0, F0, W0, p1, F1, W1)
        counts[name] = (R, T, i0, i1)
        if name != "usip64":
            g["%s_R" % name], g["%s_T" % name] = np.asarray(R), np.asarray(T).reshape(3)
            g["%s_inliers0" % name], g["%s_inliers1" % name] = np.asarray(i0), np.asarray(i1)
            g["%s_success" % name], g["%s_threshold" % name] = bool(ok), float(thr)
            from scipy.spatial.distance import cdist
            g["%s_pair_idx" % name] = np.argmin(cdist(F0, F1, metric="euclidean"), axis=0)   # Match.py:257-258
    # what carrying USIP points in float32 changes against the reference's float64
    kv = sum(int((a != b).any(axis=1).sum()) for f in FRAMES
             for a, b in zip(key_voxels(per[("usip", f)][0].astype(np.float64)), key_voxels(per[("usip64", f)][0])))
    pt = sum(int((per[("usip", f)][1] != per[("usip64", f)][1]).any(axis=2).sum()) for f in FRAMES)
    a, b = counts["usip"], counts["usip64"]
    pose = int(not (np.array_equal(np.asarray(a[0], np.float64), np.asarray(b[0], np.float64))
                    and np.array_equal(np.asarray(a[1], np.float64).ravel(), np.asarray(b[1], np.float64).ravel())))
    inl = int(not (np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])))
    g["usip_f64_changes"] = np.array([kv, pt, inl, pose])
    print("USIP float64 vs float32 (%d frames x 400 points x 3 scales): %d key voxels, %d patches, %d of 1 inlier sets, %d of 1 poses differ"
          % (len(FRAMES), kv, pt, inl, pose))
    np.savez_compressed(OUT, **g)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
