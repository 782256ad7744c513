#!/opt/conda/bin/python3.9
"""Generate tests/golden/*.npz by IMPORTING THE REFERENCE (read-only, /root/reference).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tools/make_goldens.py

Interpreter: the conda python3.9 (NumPy 1.26 = legacy type promotion like the reference's
NumPy 1.18; SciPy 1.7; scikit-learn 0.24) -- NOT the default python3 (NumPy 2 changes
Voxel.py:118-120).  Stubs: mayavi (plots), cupy -> NumPy shim with a stable
argsort (Thrust's sort is stable), np.bool alias.  Keras/TensorFlow do not exist here: the two
``model.predict`` calls are served by the oracle's restatement (PARITY UNPINNED for the CNN math,
see oracle/caelo_oracle.c), everything else is the reference's own code.

The script also asserts, stage by stage, that the oracle (oracle/oracle.py) reproduces what
the reference computed -- this is the pin.  tests/test_oracle_golden.py re-checks the oracle
against the stored fixtures without the reference.
"""
import contextlib
import hashlib
import io
import os
import sys
import time
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
cp = types.ModuleType("cupy")  # every CuPy symbol used in SphericalRing.py:137-206
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
import SphericalRing as RefSR  # noqa: E402
import Voxel as RefVoxel       # noqa: E402
import Match as RefMatch       # noqa: E402
from scipy.spatial.distance import cdist  # noqa: E402

import oracle as orc           # noqa: E402
from caelo import synth        # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
os.makedirs(GOLD, exist_ok=True)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        r = fn(*a, **k)
    return r, buf.getvalue()


resp_model, enc_model = orc.load_models(os.path.join(REPO, "weights", "SphericalRingPCRespondLayer.h5"),
                                         os.path.join(REPO, "weights", "EncoderModel4VoxelPatch.h5"))


def inconsistent_points(pc):
    """Points whose own scale-1 / scale-2 voxel index (Voxel.py:147-152) differs from their scale-0 index >> 3, >> 5
    (Voxel.py:122-143) -- computed with the reference's own float64 expressions.  Quantised clouds have some."""
    n = 0
    off = (RefVoxel.VisibleLength, RefVoxel.VisibleWidth, RefVoxel.VisibleHeight)
    for p in pc:
        if abs(p[0]) > off[0] or abs(p[1]) > off[1] or abs(p[2]) > off[2]:
            continue
        bad = False
        for a in range(3):
            x_ = p[a] + off[a]
            ib = int(x_ / RefVoxel.BlockRealSize)
            g0 = int(np.int32((x_ - ib * RefVoxel.BlockRealSize) / RefVoxel.VoxelSize)) + ib * RefVoxel.BlockSize
            bad |= int(x_ / RefVoxel.VoxelSizes[1]) != g0 >> 3 or int(x_ / RefVoxel.VoxelSizes[2]) != g0 >> 5
        n += bad
    return n


def frame_golden(frame, n_beams=64, n_az=2000, n_patch_kp=None, tag=None, quantum=None, scene_kind="boxes", shuffle_seed=None):
    t0 = time.time()
    g = {}
    pc = synth.make_scan(frame, n_beams=n_beams, n_az=n_az, quantum=quantum, scene_kind=scene_kind)
    if shuffle_seed is not None:
        # hostile file order (round 4): 1 % of the points repeated with another intensity, everything permuted -- the
        # last-writer-wins rule of SphericalRing.py:91-93 and the first-touch rule of Voxel.py:139-158 across distant positions
        ordered = pc
        pc = synth.shuffle_scan(pc, shuffle_seed)
        g["shuffle_seed"] = shuffle_seed
        ring_a, _ = RefSR.ProjectPC2SphericalRing(ordered)
        ring_b, _ = RefSR.ProjectPC2SphericalRing(pc)
        g["ring_pixels_changed_by_order"] = int((ring_a != ring_b).any(axis=2).sum())
        va, vb = RefVoxel.Voxelization(ordered[:, 0:3]), RefVoxel.Voxelization(pc[:, 0:3])
        g["voxel_lists_reordered"] = np.array([not np.array_equal(va[6 + s_], vb[6 + s_]) for s_ in range(3)])
        g["voxel1_set_changed_by_order"] = bool({tuple(r) for r in va[7]} != {tuple(r) for r in vb[7]})
        print("  frame %s: order changes %d ring pixels, voxel lists reordered %s, scale-1 SET changed %s" % (
            tag, g["ring_pixels_changed_by_order"], g["voxel_lists_reordered"], g["voxel1_set_changed_by_order"]))
    if quantum:
        g["quantum"] = quantum
        g["n_inconsistent_points"] = inconsistent_points(pc)
        print("  frame %s: %d points on voxel faces (scale-1/2 index != scale-0 index >> 3/5)" % (tag, g["n_inconsistent_points"]))
    g["cloud_sha256"] = synth.cloud_sha256(pc)
    g["n_points"] = pc.shape[0]
    g["scan_params"] = np.array([frame, n_beams, n_az])
    # -- projection (reference) vs oracle
    ring, cnt = RefSR.ProjectPC2SphericalRing(pc)
    o_ring, o_cnt = orc.ProjectPC2SphericalRing(pc)
    assert np.array_equal(ring, o_ring) and np.array_equal(cnt, o_cnt), "oracle projection != reference"
    g["ring_sha256"], g["counter_sha256"] = sha(ring), sha(cnt)
    g["counter_nnz"] = int((cnt > 0).sum()); g["counter_max"] = int(cnt.max())
    g["counter_bits"] = np.packbits(cnt > 0)
    # -- response image: oracle restatement of the Keras layer (unpinned)
    x = ring[0:64, 0:1792, :][:, :, [0, 1, 2]]
    resp = np.squeeze(resp_model.predict(x.reshape(1, 64, 1792, 3)))
    g["respond_sha256"] = sha(resp)
    g["respond_sample"] = resp[20:24, 100:132, :].copy()
    # -- keypoints (reference, both calling modes) vs oracle
    (kp_d, kpix_d, _), _ = quiet(RefSR.GetKeyPtsByAE, ring, cnt, resp)
    ring_b = np.ascontiguousarray(ring[0:64, 0:1792, :][:, :, [0, 1, 2]])
    cnt_b = np.array(cnt[0:64, 0:1792], dtype=np.int8)  # BatchPreprocess.py:98
    (kp_b, kpix_b, _), _ = quiet(RefSR.GetKeyPtsByAE, ring_b, cnt_b, resp)
    o_kp, o_kpix, _ = orc.GetKeyPtsByAE(ring, cnt, resp)
    assert np.array_equal(o_kpix, kpix_d) and np.array_equal(o_kp, kp_d), "oracle keypoints (demo) != reference"
    o_kp2, o_kpix2, _ = orc.GetKeyPtsByAE(ring_b, cnt_b.astype(np.int32), resp)
    assert np.array_equal(o_kpix2, kpix_b) and np.array_equal(o_kp2, kp_b), "oracle keypoints (batch) != reference"
    g["keypixels_demo"] = kpix_d.astype(np.int16); g["keypixels_batch"] = kpix_b.astype(np.int16)
    g["keypts_demo"] = kp_d.astype(np.float32)
    print("  frame %s: K=%d/%d shared=%d  (%.1fs)" % (tag or frame, len(kpix_d), len(kpix_b),
          len(set(map(tuple, kpix_d)) & set(map(tuple, kpix_b))), time.time() - t0))
    # -- voxelization (reference) vs oracle
    tv = time.time()
    vout = RefVoxel.Voxelization(pc[:, 0:3])
    A0, A1, A2 = vout[6], vout[7], vout[8]
    o = orc.Voxelization(pc[:, 0:3])
    for a, b, nm in ((A0, o[6], "AllVoxels0"), (A1, o[7], "AllVoxels1"), (A2, o[8], "AllVoxels2")):
        assert a.dtype == np.int16 and np.array_equal(a, b), "oracle %s != reference" % nm
    g["voxel_counts"] = np.array([len(A0), len(A1), len(A2)])
    g["voxels0_sha256"], g["voxels1_sha256"], g["voxels2_sha256"] = sha(A0), sha(A1), sha(A2)
    g["voxels2"] = A2  # small: keep one full list as a fixture
    if quantum:
        g["voxels1"] = A1  # the scale the face points perturb most
    print("    voxels %s (%.1fs)" % (g["voxel_counts"], time.time() - tv))
    # -- patches (reference) vs oracle
    kp = kp_d if n_patch_kp is None else kp_d[-n_patch_kp:]
    tp = time.time()
    _, plist = RefVoxel.GetPatchesList(kp, A0, A1, A2)
    bits = np.stack([orc.pack_patches(p) for p in plist], axis=1)  # [K,3,64]
    o_bits, o_flags = [], []
    for s, A in enumerate((A0, A1, A2)):
        b, f = orc.patches_bits(kp, A, s)
        o_bits.append(b); o_flags.append(f)
    o_bits = np.stack(o_bits, 1); o_flags = np.stack(o_flags, 1)
    diff = (o_bits != bits).any(axis=2)
    amb = (o_flags & 2) != 0
    assert not (diff & ~amb).any(), "oracle patches != reference on a non-ambiguous patch"
    assert not amb.any(), "scan-sized voxel lists are kd-tree sized: no patch may be left to the canonical rule"
    g["patch_bits"] = bits; g["patch_flags"] = o_flags
    g["patch_kp"] = kp.astype(np.float32)
    print("    patches: set voxels mean %s, truncated %s, cut inside a tie class (kd-tree order) %s, differ %d (%.1fs)" % (
        np.round(np.unpackbits(bits.view(np.uint8), axis=2).sum(axis=2).mean(axis=0), 1),
        ((o_flags & 1) != 0).sum(axis=0), ((o_flags & 4) != 0).sum(axis=0), int(diff.sum()), time.time() - tp))
    # -- descriptors: oracle restatement of the Keras encoder on the reference's patches
    feats = RefMatch.GetFeaturesFromPatches(enc_model, plist)
    g["features"] = feats.astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "frame_%s.npz" % (tag or frame)), **g)
    return dict(pc=pc, kp=kp_d, feats=feats, A=(A0, A1, A2))


def pair_golden(f0, f1, seeds=(0, 1, 2, 3), out="pair_0_1.npz", hard_cases=True):
    g = {}
    kp0, F0, kp1, F1 = f0["kp"], f0["feats"], f1["kp"], f1["feats"]
    W0 = np.ones((kp0.shape[0], 1), np.float32); W1 = np.ones((kp1.shape[0], 1), np.float32)
    D = cdist(F0, F1, metric="euclidean")
    pairIdx = np.argmin(D, axis=0)
    o_idx, o_dist = orc.match(F0, F1)
    assert np.array_equal(o_idx, pairIdx) and np.array_equal(o_dist, D.min(axis=0)), "oracle match != reference"
    g["pair_idx"] = pairIdx.astype(np.int32)
    part = np.partition(D, 1, axis=0)
    g["match_margin_min"] = float(((part[1] - part[0]) / part[0]).min())
    for s in seeds:
        np.random.seed(s)
        (R, T, ok, i0, i1, thr), log = quiet(RefMatch.SolveRelativePose, kp0, F0, W0, kp1, F1, W1)
        iters = int(log.split("cntItersRANSAC =")[1].split()[0])
        trace = []
        oR, oT, ook, oi0, oi1, othr = orc.SolveRelativePose(kp0, F0, W0, kp1, F1, W1,
                                                             rng=np.random.RandomState(s), trace=trace)
        assert ook == ok and othr == thr and np.array_equal(oi0, i0) and np.array_equal(oi1, i1)
        assert np.allclose(oR, R, atol=1e-6) and np.allclose(oT, T, atol=1e-5), "oracle pose != reference"
        g["s%d_R" % s] = np.asarray(R, np.float64); g["s%d_T" % s] = np.asarray(T, np.float64)
        g["s%d_ok" % s] = bool(ok); g["s%d_thr" % s] = float(thr); g["s%d_iters" % s] = iters
        g["s%d_idx0" % s] = i0.astype(np.int32); g["s%d_idx1" % s] = i1.astype(np.int32)
        g["s%d_trace_idx" % s] = np.array([t[0] for t in trace], np.int32)
        g["s%d_trace_cnt" % s] = np.array([t[1] for t in trace], np.int32)
        print("  pair seed %d: ok=%s thr=%.1f iters=%d inliers=%d T=%s" % (s, ok, thr, iters, len(i0), np.round(T.ravel(), 3)))
    if not hard_cases:
        np.savez_compressed(os.path.join(GOLD, out), **g)
        return
    # hard cases: few correspondences -> escalation / failure (Match.py:207-214)
    rs = np.random.RandomState(99)
    P1 = rs.uniform(-30, 30, (300, 3)).astype(np.float32)
    Rg, Tg = synth.relative_pose_gt(0, 1)
    for name, frac, noise in (("esc", 0.8, 0.45), ("fail", 0.0, 0.0)):
        P0 = (P1 @ Rg.T + Tg.T).astype(np.float32)
        bad = rs.uniform(size=300) >= frac
        P0[bad] = rs.uniform(-30, 30, (int(bad.sum()), 3)).astype(np.float32)
        P0 += rs.normal(0, noise, P0.shape).astype(np.float32)
        np.random.seed(7)
        (R, T, ok, mask, thr), log = quiet(RefMatch.RANSAC4RT, P0, P1, None, None)
        oR, oT, ook, omask, othr = orc.RANSAC4RT(P0, P1, rng=np.random.RandomState(7))
        assert ook == ok and othr == thr and np.array_equal(omask, mask)
        g[name + "_P0"] = P0; g[name + "_P1"] = P1; g[name + "_ok"] = bool(ok); g[name + "_thr"] = float(thr)
        g[name + "_mask"] = np.asarray(mask, bool); g[name + "_R"] = np.asarray(R, np.float64); g[name + "_T"] = np.asarray(T, np.float64)
        print("  ransac %s: ok=%s thr=%.1f inliers=%d" % (name, ok, thr, int(np.sum(mask))))
    np.savez_compressed(os.path.join(GOLD, out), **g)


def quantised_golden():
    """mm-quantised scans (KITTI-style values): points exactly on voxel faces, where the reference's float64 index
    arithmetic decides which scale-1 / scale-2 voxel a scale-0 voxel's first point marks (Voxel.py:139-158)."""
    q0 = frame_golden(0, quantum=1e-3, tag="q0")
    q1 = frame_golden(1, quantum=1e-3, tag="q1")
    pair_golden(q0, q1, seeds=(0, 1), out="pair_q0_q1.npz", hard_cases=False)


def clutter_golden():
    """Round 3: the second scene (synth.make_scan(scene_kind="clutter"): trees and bushes made of spheres, mm-quantised) through
    the reference -- dense 16 cm / 64 cm patches, the 496-nearest cut of Voxel.py:182,195-196 on REAL key points, few equal
    patches."""
    c0 = frame_golden(0, quantum=1e-3, tag="c0", scene_kind="clutter")
    c1 = frame_golden(1, quantum=1e-3, tag="c1", scene_kind="clutter")
    pair_golden(c0, c1, seeds=(0, 1), out="pair_c0_c1.npz", hard_cases=False)


def tie_golden():
    """Round 4: a REAL frame whose 496-nearest cut falls inside classes of equidistant voxels (clutter frame 23: 3 patches at
    16 cm, 8 at 64 cm; 17 truncated in all): the reference's patches, which the oracle reproduces in scikit-learn's kd-tree order."""
    frame_golden(23, quantum=1e-3, tag="c23", scene_kind="clutter")


def shuffled_golden():
    """Round 4 (missing 4): frame 0 of the mm-quantised scene in a hostile file order through the reference."""
    frame_golden(0, quantum=1e-3, tag="p0", shuffle_seed=77)


def trunc_golden():
    """Crafted dense voxel clouds: force the 496-NN cap of Voxel.py:182,195-196 to bite."""
    g = {}
    rs = np.random.RandomState(5)
    c = np.array([600, 640, 90])
    for name, p in (("sparse", 0.04), ("mid", 0.12), ("dense", 0.45)):
        occ = rs.uniform(size=(40, 40, 40)) < p
        vox = (np.argwhere(occ) + (c - 20)).astype(np.int16)
        vox = vox[rs.permutation(len(vox))]
        kv = c + rs.randint(-5, 6, size=(48, 3))
        pts = (kv * 0.16 - orc.VIS + rs.uniform(0.01, 0.15, size=(48, 3))).astype(np.float32)
        _, plist = RefVoxel.GetPatchesList(pts, vox, vox, vox)
        bits = orc.pack_patches(plist[1])
        ob, of = orc.patches_bits(pts, vox, 1)
        diff = (ob != bits).any(axis=1); amb = (of & 2) != 0
        assert not (diff & ~amb).any(), "oracle truncated patches != reference (outside the brute-force case)"
        assert len(vox) < 994 or not amb.any(), "a kd-tree sized list left a patch to the canonical rule"
        # round 4: the cut inside a class of equidistant voxels is resolved in scikit-learn's kd-tree order (flag 4): EVERY patch equal
        print("  trunc %-6s: nvox=%d truncated=%d kd-tree-ordered=%d canonical(brute-force case)=%d differ=%d setbits ref/oracle=%d/%d" % (
            name, len(vox), int(((of & 1) != 0).sum()), int(((of & 4) != 0).sum()), int(amb.sum()), int(diff.sum()),
            int(np.unpackbits(bits.view(np.uint8)).sum()), int(np.unpackbits(ob.view(np.uint8)).sum())))
        g[name + "_vox"] = vox; g[name + "_pts"] = pts; g[name + "_bits"] = bits; g[name + "_flags"] = of
    # the tree itself against the library: index array of KDTree(leaf_size=30) and raw 496-neighbour sets on lattices full of ties
    from sklearn.neighbors import KDTree, NearestNeighbors
    n_q = n_same = 0
    for trial in range(24):
        side = rs.randint(9, 40)
        X = np.unique(rs.randint(0, side, size=(rs.randint(1200, 9000), 3)), axis=0).astype(np.int16)
        X = X[rs.permutation(len(X))] + np.int16(100)
        if len(X) < 994:
            continue
        idx, n_nodes = orc.kdtree_idx(X)
        sk = KDTree(X.astype(np.float64), leaf_size=30).get_arrays()
        assert np.array_equal(idx, sk[1]) and n_nodes == len(sk[2]), "oracle kd-tree != scikit-learn's (index array)"
        nn = NearestNeighbors(n_neighbors=496, radius=14, algorithm="auto").fit(X)
        assert nn._fit_method == "kd_tree"
        Q = X[rs.randint(0, len(X), 40)].astype(np.int32) + rs.randint(-2, 3, size=(40, 3))
        ref = nn.kneighbors(Q, return_distance=False)
        got = orc.kdtree_query(X, Q)
        n_q += len(Q); n_same += sum(set(a.tolist()) == set(b.tolist()) for a, b in zip(ref, got))
    assert n_q == n_same and n_q >= 400, "oracle kd-tree query != scikit-learn's kneighbors (as sets)"
    g["kdtree_checked_queries"] = n_q
    # below 994 voxels 'auto' is brute force (np.argpartition's order: brute_golden)
    small = NearestNeighbors(n_neighbors=496, radius=14, algorithm="auto").fit(g["sparse_vox"][:993])
    assert small._fit_method == "brute" and NearestNeighbors(n_neighbors=496, algorithm="auto").fit(g["sparse_vox"][:994])._fit_method == "kd_tree"
    print("  kd-tree: %d lattice queries equal to scikit-learn %s as sets; index arrays equal" % (n_q, __import__("sklearn").__version__))
    np.savez_compressed(os.path.join(GOLD, "patch_truncation.npz"), **g)


def brute_golden():
    """Round 6 (missing 4): voxel lists of 496 .. 993 entries, where NearestNeighbors(algorithm='auto') is brute force and
    the members of a split tie class are chosen by np.argpartition (Voxel.py:182,195-196).  (1) the oracle's introselect against
    np.argpartition of THIS interpreter's NumPy (1.26: the reference's algorithm) as full permutations; (2) the oracle's raw
    496-neighbour sets against scikit-learn's brute kneighbors; (3) the reference's GetPatchesList on crafted short lists."""
    from sklearn.neighbors import NearestNeighbors
    assert np.__version__.startswith("1."), "np.argpartition of NumPy >= 2 is another algorithm on AVX-512 hosts"
    g = {}
    rs = np.random.RandomState(11)
    rows, perms = [], []
    for it in range(36):
        n = int(rs.randint(496, 994)) if it else 993
        mode = it % 6
        if mode == 0: v = rs.randint(0, 8, n)
        elif mode == 1: v = rs.randint(0, 200, n)
        elif mode == 2: v = np.sort(rs.randint(0, 50, n))
        elif mode == 3: v = np.sort(rs.randint(0, 50, n))[::-1]
        elif mode == 4: v = (rs.randint(-9, 10, (n, 3)) ** 2).sum(1)
        else: v = np.r_[np.arange(n // 2), np.arange(n - n // 2)[::-1]]   # organ pipe: the median-of-medians fallback runs
        ref = np.argpartition(v.astype(np.float64), 495)
        assert np.array_equal(ref, orc.argpartition(v, 495)), "oracle introselect != np.argpartition"
        rows.append(np.asarray(v, np.int16)); perms.append(ref.astype(np.int16))
    n_any = 0
    for it in range(4000):   # not stored: any kth, any length
        n = int(rs.randint(2, 3000)); kth = int(rs.randint(0, n))
        v = (rs.randint(0, 5, n), rs.randint(0, 10 ** 6, n), np.r_[np.arange(n // 2), np.arange(n - n // 2)[::-1]], np.arange(n)[::-1] // 3)[it % 4]
        assert np.array_equal(np.argpartition(v.astype(np.float64), kth), orc.argpartition(v, kth))
        n_any += 1
    g["rows"] = np.concatenate(rows); g["perms"] = np.concatenate(perms); g["row_len"] = np.array([len(r) for r in rows], np.int32)
    g["checked_rows_any_kth"] = n_any
    c = np.array([600, 640, 90])
    n_q = n_same = 0
    for name, n_vox, side in (("ball", 990, 0), ("cube", 729, 9), ("slab", 993, 0), ("min", 496, 0)):
        if name == "ball":      # the 990 nearest cells of a dense lattice: every distance class is large
            lat = np.argwhere(np.ones((15, 15, 15), bool)) - 7
            lat = lat[np.argsort((lat ** 2).sum(1), kind="stable")[:n_vox]]
        elif name == "cube":
            lat = np.argwhere(np.ones((side, side, side), bool)) - side // 2
        elif name == "slab":    # two dense layers: what a wall is at 64 cm
            lat = np.argwhere(np.ones((24, 24, 2), bool)) - np.array([12, 12, 0])
            lat = lat[rs.permutation(len(lat))[:n_vox]]
        else:
            lat = np.argwhere(rs.uniform(size=(12, 12, 12)) < 0.5) - 6
            lat = lat[:n_vox]
        vox = (lat[rs.permutation(len(lat))] + c).astype(np.int16)
        assert len(vox) == n_vox
        nn = NearestNeighbors(n_neighbors=496, radius=14, algorithm="auto").fit(vox)
        assert nn._fit_method == "brute"
        kv = c + rs.randint(-3, 4, size=(48, 3))
        ref = nn.kneighbors(kv.astype(np.int32), return_distance=False)
        got = orc.brute_query(vox, kv)
        n_q += len(kv); n_same += sum(set(a.tolist()) == set(b.tolist()) for a, b in zip(ref, got))
        pts = (kv * 0.16 - orc.VIS + rs.uniform(0.01, 0.15, size=(48, 3))).astype(np.float32)
        _, plist = RefVoxel.GetPatchesList(pts, vox, vox, vox)
        bits = orc.pack_patches(plist[1])
        ob, of = orc.patches_bits(pts, vox, 1)
        assert np.array_equal(ob, bits) and not (of & 2).any(), "oracle patches != reference on a brute-force sized list"
        print("  brute %-5s: nvox=%d truncated=%d argpartition-ordered=%d setbits %d" % (
            name, len(vox), int(((of & 1) != 0).sum()), int(((of & 4) != 0).sum()), int(np.unpackbits(bits.view(np.uint8)).sum())))
        g[name + "_vox"] = vox; g[name + "_pts"] = pts; g[name + "_bits"] = bits; g[name + "_flags"] = of
    assert n_q == n_same, "oracle brute query != scikit-learn's kneighbors (as sets)"
    g["brute_checked_queries"] = n_q
    print("  brute force: %d rows equal to np.argpartition %s (+%d of any kth), %d queries equal to scikit-learn %s as sets" % (
        len(rows), np.__version__, n_any, n_q, __import__("sklearn").__version__))
    np.savez_compressed(os.path.join(GOLD, "patch_brute.npz"), **g)


def extend_golden():
    """ExtendKeyPtsInShpericalRing (SphericalRing.py:294-317) in both calling modes on frame 0: the reference's output
    and its in-place edit of GridCounter; the oracle restatement is asserted equal."""
    pc = synth.make_scan(0)
    ring, cnt = RefSR.ProjectPC2SphericalRing(pc)
    resp = np.squeeze(resp_model.predict(ring[0:64, 0:1792, :][:, :, [0, 1, 2]].reshape(1, 64, 1792, 3)))
    g = {}
    for mode in ("demo", "batch"):
        if mode == "demo":
            r, c = ring.copy(), cnt.copy()
        else:   # BatchPreprocess.py:97-98,131-139: cropped 3-channel ring, int8 counter of the full image
            r, c = np.ascontiguousarray(ring[0:64, 0:1792, :][:, :, [0, 1, 2]]), np.array(cnt, dtype=np.int8)
        (kp, kpix, _), _ = quiet(RefSR.GetKeyPtsByAE, r, c[0:64, 0:1792] if mode == "batch" else c, resp)
        c_ref, c_orc = c.copy(), c.copy()
        ext = RefSR.ExtendKeyPtsInShpericalRing(r, c_ref, kpix)
        o_ext = orc.ExtendKeyPtsInShpericalRing(r, c_orc, kpix)
        assert np.array_equal(ext, o_ext) and np.array_equal(c_ref, c_orc), "oracle ExtendKeyPts != reference"
        g[mode + "_keypixels"] = kpix.astype(np.int16)
        g[mode + "_n_ext"] = len(ext); g[mode + "_ext_sha256"] = sha(np.asarray(ext, np.float32))
        g[mode + "_ext_head"] = np.asarray(ext[:64], np.float32); g[mode + "_ext_tail"] = np.asarray(ext[-64:], np.float32)
        g[mode + "_counter_after_sha256"] = sha(np.asarray(c_ref, np.int32)); g[mode + "_counter_after_nnz"] = int((c_ref > 0).sum())
        print("  extend golden (%s): %d points from %d keypixels, counter nnz %d -> %d" % (
            mode, len(ext), len(kpix), int((c > 0).sum()), int((c_ref > 0).sum())))
    np.savez_compressed(os.path.join(GOLD, "extend_0.npz"), **g)


def icp_golden():
    """MyICP.ICP (MyICP.py:26-72) on the extended keypoints of frames 0 and 1, frame 1 pre-aligned with the odometry
    pose of pair_0_1.npz (seed 0) like RefinePoses.py:283-284; the oracle restatement (brute-force float64 nearest
    neighbours instead of sklearn's kd-tree) is asserted against it."""
    import MyICP as RefICP
    pair = np.load(os.path.join(GOLD, "pair_0_1.npz"))
    ext = []
    for f in (0, 1):
        pc = synth.make_scan(f)
        ring, cnt = RefSR.ProjectPC2SphericalRing(pc)
        resp = np.squeeze(resp_model.predict(ring[0:64, 0:1792, :][:, :, [0, 1, 2]].reshape(1, 64, 1792, 3)))
        (kp, kpix, _), _ = quiet(RefSR.GetKeyPtsByAE, ring, cnt, resp)
        ext.append(np.asarray(RefSR.ExtendKeyPtsInShpericalRing(ring, cnt, kpix), np.float32))
    R, T = pair["s0_R"], pair["s0_T"].reshape(3, 1)
    pc1_ = np.array((np.dot(R, ext[1].T) + T).T, dtype=np.float32)            # RefinePoses.py:284
    (Rs, Ts, ok), log = quiet(RefICP.ICP, ext[0], pc1_)
    trace = []
    oR, oT, ook = orc.ICP(ext[0], pc1_, trace=trace)
    iters = int(log.split("ICP iters:")[1].split(",")[0]); inl = int(log.split("inliers:")[1].split(",")[0])
    assert ook == ok and len(trace) == iters and trace[-1][0] == inl, (len(trace), iters, trace[-1], inl)
    assert np.allclose(oR, Rs, atol=1e-7) and np.allclose(oT, Ts, atol=1e-6), "oracle ICP != reference"
    g = {"n_ext": np.array([len(ext[0]), len(ext[1])]), "ext0_sha256": sha(ext[0]), "pc1_sha256": sha(pc1_),
         "R_odo": R, "T_odo": T, "R_star": np.asarray(Rs, np.float64), "T_star": np.asarray(Ts, np.float64), "success": bool(ok),
         "iters": iters, "inliers_last": inl, "trace_inliers": np.array([t[0] for t in trace], np.int32),
         "trace_thr": np.array([t[1] for t in trace], np.float64)}
    np.savez_compressed(os.path.join(GOLD, "icp_0_1.npz"), **g)
    print("  icp golden: %d iterations, %d inliers, ok=%s, T_star=%s" % (iters, inl, ok, np.round(np.asarray(Ts).ravel(), 4)))


def icp_loop_golden():
    """The reference's two loops on the crafted clouds of tests/icp_clouds.py: MyICP.ICP on `points`, `points_102` (102
    iterations: MyICP.ICP has no branch at iteration 100) and `late_fail` (too few pairs at a late iteration), MyICP.ICP_Pt2PtAndPt2Plane on `planar`, `planar_late_stop` (too few pairs after the first
    iteration: success, loop ended) and `planar_103` (103 iterations: the branch of MyICP.py:151-153 that fits the planar
    pairs of iteration 99 again and again).  The oracle is asserted against each; stored are the results, the parameters and
    the SHA-256 of every input array -- the arrays themselves are rebuilt from their seeds."""
    import json
    import MyICP as RefICP
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import icp_clouds
    g = {"cases": np.array(sorted(icp_clouds.CASES))}
    for name in sorted(icp_clouds.CASES):
        loop, kw = icp_clouds.CASES[name][1], icp_clouds.loop_kw(name)
        arrays = icp_clouds.clouds(name)
        fn = RefICP.ICP if loop == "icp" else RefICP.ICP_Pt2PtAndPt2Plane
        (Rs, Ts, ok), log = quiet(fn, *[a.copy() for a in arrays], **kw)
        oR, oT, ook, steps = icp_clouds.run_oracle(orc, name)
        iters = int(log.split("ICP iters:")[1].split(",")[0])
        if loop == "icp":
            counts = (int(log.split("inliers:")[1].split(",")[0]), 0)
            thr = (float(log.split("inlierThreshold:")[1]), 0.0)
        else:
            counts = (int(log.split("inliers0:")[1].split(",")[0]), int(log.split("inliers1:")[1].split(",")[0]))
            thr = (float(log.split("th0:")[1].split(",")[0]), float(log.split("th1:")[1]))
        last = steps[-1]
        assert ook == ok and len(steps) == iters and (last["n_pts"], last["n_planar"]) == counts, (name, ook, ok, len(steps), iters, last, counts)
        assert (round(last["thr0"], 5), round(last["thr1"], 5)) == thr, (name, last, thr)
        assert np.allclose(oR, Rs, atol=1e-7) and np.allclose(oT, Ts, atol=1e-6), "oracle != reference on %s: T %s vs %s" % (name, np.ravel(oT), np.ravel(Ts))
        margin = min(s["margin"] for s in steps)
        assert margin >= icp_clouds.GATE_MARGIN, (name, margin)
        g.update({name + "_R_star": np.asarray(Rs, np.float64), name + "_T_star": np.asarray(Ts, np.float64).reshape(3), name + "_success": bool(ok),
                  name + "_iters": iters, name + "_moves": last["iterations"], name + "_counts": np.array(counts, np.int32),
                  name + "_thr": np.array(thr, np.float64), name + "_kw": json.dumps(kw, sort_keys=True),
                  name + "_sha256": np.array([sha(a) for a in arrays])})
        print("  icp loop golden %-16s: %3d iterations, pairs %d + %d, ok=%s, margin %.2e, T_star=%s"
              % (name, iters, counts[0], counts[1], ok, margin, np.round(np.asarray(Ts).ravel(), 4)))
    np.savez_compressed(os.path.join(GOLD, "icp_loop.npz"), **g)


def refine_golden():
    """SURVEY 8f-4, the rest: MyICP.ICP_Pt2PtAndPt2Plane (MyICP.py:127-201) and RefinePoses.RefinementCore
    (RefinePoses.py:273-334, with ForwardUpdatePoses :120-145) run by the reference itself.
    * With what the reference's own pipeline stores -- GetKeyPtsByAE returns an EMPTY PlanarPts (SphericalRing.py:219,285) --
      ICP_Pt2PtAndPt2Plane raises (sklearn refuses to fit an empty set, MyICP.py:94): recorded.
    * With planar points given (ground returns of the synthetic scans with their normal), both run; the oracle restatements are
      asserted against them.  RefinePoses.py cannot be imported (it executes a script at module level): the two function
      definitions are executed from its source into a namespace that provides what they use."""
    import copy
    import MyICP as RefICP
    import Transformations as RefT
    pair = np.load(os.path.join(GOLD, "pair_0_1.npz"))
    seq = np.load(os.path.join(GOLD, "sequence_20.npz"))
    ext, planar = [], []
    for f in (0, 1):
        pc = synth.make_scan(f)
        ring, cnt = RefSR.ProjectPC2SphericalRing(pc)
        resp = np.squeeze(resp_model.predict(ring[0:64, 0:1792, :][:, :, [0, 1, 2]].reshape(1, 64, 1792, 3)))
        (kp, kpix, _), _ = quiet(RefSR.GetKeyPtsByAE, ring, cnt, resp)
        ext.append(np.asarray(RefSR.ExtendKeyPtsInShpericalRing(ring, cnt, kpix), np.float32))
        g_ = pc[(pc[:, 2] < -1.6) & (np.abs(pc[:, 0]) < 30) & (np.abs(pc[:, 1]) < 30)][::9, 0:3]       # ground returns near the sensor
        planar.append(np.ascontiguousarray(np.c_[g_, np.tile(np.array([[0, 0, 1]], np.float32), (len(g_), 1))], np.float32))
    assert planar[1].shape[0] > 2000, planar[1].shape       # exercises the random subsampling at MyICP.py:135-140
    g = {"planar_stride": 9, "n_planar": np.array([len(planar[0]), len(planar[1])]), "n_ext": np.array([len(ext[0]), len(ext[1])])}
    # ---- (1) empty planar points: what the reference's own artefacts lead to
    e0 = np.zeros((0, 0), np.float32)
    try:
        quiet(RefICP.ICP_Pt2PtAndPt2Plane, ext[0], ext[1], e0, e0)
        raise AssertionError("the reference was expected to raise on empty planar points")
    except ValueError as ex:
        g["empty_planar_exception"] = "ValueError: " + str(ex)
    try:
        orc.ICP_Pt2PtAndPt2Plane(ext[0], ext[1], e0, e0)
        raise AssertionError("oracle did not raise")
    except ValueError:
        pass
    # ---- (2) ICP_Pt2PtAndPt2Plane with RefinementCore's parameters (:290-293), frame 1 pre-aligned by the odometry pose
    R, T = pair["s0_R"], pair["s0_T"].reshape(3, 1)
    pc1_ = np.array((np.dot(R, ext[1].T) + T).T, dtype=np.float32)
    pn1_ = planar[1].copy(); pn1_[:, 0:3] = np.array((np.dot(R, planar[1][:, 0:3].T) + T).T, dtype=np.float32)
    kw = dict(maxIterTimes=50, minIterTimes=20 - 1, inlierThreshold0=0.5, decay_rate0=0.9, inlierThreshold1=5.0, decay_rate1=0.9,
              smallShiftThreshold=0.1, ep=0.001)
    np.random.seed(3)
    (Rs, Ts, ok), log = quiet(RefICP.ICP_Pt2PtAndPt2Plane, ext[0], pc1_.copy(), planar[0], pn1_.copy(), **kw)
    trace = []
    oR, oT, ook = orc.ICP_Pt2PtAndPt2Plane(ext[0], pc1_.copy(), planar[0], pn1_.copy(), rng=np.random.RandomState(3), trace=trace, **kw)
    iters = int(log.split("ICP iters:")[1].split(",")[0]); in0 = int(log.split("inliers0:")[1].split(",")[0]); in1 = int(log.split("inliers1:")[1].split(",")[0])
    assert ook == ok and len(trace) == iters and trace[-1][0] == in0 and trace[-1][1] == in1, (len(trace), iters, trace[-1], in0, in1)
    assert np.allclose(oR, Rs, atol=1e-7) and np.allclose(oT, Ts, atol=1e-6), "oracle ICP_Pt2PtAndPt2Plane != reference"
    g.update(R_odo=R, T_odo=T, p2p_R_star=np.asarray(Rs, np.float64), p2p_T_star=np.asarray(Ts, np.float64), p2p_success=bool(ok),
             p2p_iters=iters, p2p_trace=np.array(trace, np.float64), p2p_seed=3)
    print("  refine golden: Pt2Pt+Pt2Plane %d iterations, inliers %d + %d, ok=%s, T_star=%s" % (iters, in0, in1, ok, np.round(np.asarray(Ts).ravel(), 4)))
    # ---- (3) RefinementCore: the reference's function executed from its source
    src = ref_source_block(os.path.join(REF, "RefinePoses.py"), 120, 145) + "\n\n" + ref_source_block(os.path.join(REF, "RefinePoses.py"), 273, 334)
    tr = seq["tr_kitti"].astype(np.float64)
    R_Tr, T_Tr = RefT.GetRtFromOnePose(tr)
    R_Tr_inv = np.linalg.inv(R_Tr); T_Tr_inv = -np.dot(R_Tr_inv, T_Tr)
    ns = {k: getattr(RefT, k) for k in dir(RefT) if not k.startswith("_")}
    ns.update(np=np, LA=np.linalg, copy=copy, dot=np.dot, ICP_Pt2PtAndPt2Plane=lambda *a, **k: quiet(RefICP.ICP_Pt2PtAndPt2Plane, *a, **k)[0],
              LoadExtendedKeyPts=lambda strSequence, iFrame: (ext[iFrame], planar[iFrame]), R_Tr=R_Tr, T_Tr=T_Tr, R_Tr_inv=R_Tr_inv,
              T_Tr_inv=T_Tr_inv, iShowMatchingResult=0, print=lambda *a, **k: None)
    exec(src, ns)
    poses = seq["poses_kitti"].astype(np.float64)
    relRs = np.zeros((len(poses) - 1, 3, 3)); relTs = np.zeros((len(poses) - 1, 3))
    for i in range(len(poses) - 1):
        r_, t_ = RefT.GetRelRtBetween2Poses(poses[i], poses[i + 1])
        relRs[i], relTs[i] = r_, t_.reshape(3,)
    np.random.seed(4)
    flag, poses_, relRs_, relTs_ = ns["RefinementCore"](poses, "00", 0, 1, relRs, relTs, 0.5)
    oflag, oposes, orelRs, orelTs = orc.RefinementCore(poses, ext[0], planar[0], ext[1], planar[1], 0, 1, relRs, relTs, 0.5, tr, rng=np.random.RandomState(4))
    assert oflag == flag == 1, (oflag, flag)
    assert np.allclose(oposes, poses_, atol=1e-6) and np.allclose(orelRs, relRs_, atol=1e-7) and np.allclose(orelTs, relTs_, atol=1e-6), "oracle RefinementCore != reference"
    g.update(rc_flag=int(flag), rc_poses_in=poses, rc_poses_out=np.asarray(poses_), rc_relRs_in=relRs, rc_relTs_in=relTs, rc_relRs_out=np.asarray(relRs_),
             rc_relTs_out=np.asarray(relTs_), rc_tr=tr, rc_seed=4)
    print("  refine golden: RefinementCore flag %d, pose1 T %s -> %s" % (flag, np.round(poses[1].reshape(3, 4)[:, 3], 4), np.round(np.asarray(poses_)[1].reshape(3, 4)[:, 3], 4)))
    np.savez_compressed(os.path.join(GOLD, "refine_0_1.npz"), **g)


def blocks_golden():
    """Voxel.py:161-172 block structures (written to VoxelModel/*.mat, BatchVoxelization.py:61-62) of a small scan: pins
    caelo.stageio.block_structures, which derives them from AllVoxels0 alone."""
    pc = synth.make_scan(3, n_beams=16, n_az=600)
    out = RefVoxel.Voxelization(pc[:, 0:3])
    g = {"scan_params": np.array([3, 16, 600]), "avlBlocksList": out[3], "cntVoxelsLength": out[4], "AllVoxels": out[5],
         "AllVoxels0": out[6], "AllVoxels1": out[7], "AllVoxels2": out[8]}
    assert out[3].dtype == np.int16 and out[4].dtype == np.int32 and out[5].dtype == np.int16
    # tuple members 0-2 (Voxel.py:101-107,:126-158): VoxelModel1/2 as shapes + dtype + occupied cells (argwhere order), Blocks
    # through three occupied blocks (dense 64^3 int8 occupancy as argwhere, local and global voxel lists) and one empty one
    Blocks, VM1, VM2 = out[0], out[1], out[2]
    g["vm1_shape"], g["vm2_shape"] = np.array(VM1.shape), np.array(VM2.shape)
    g["vm_dtype"] = str(VM1.dtype)
    assert VM1.dtype == VM2.dtype == np.int8 and set(np.unique(VM1)) <= {0, 1}
    g["vm1_nz"], g["vm2_nz"] = np.argwhere(VM1).astype(np.int16), np.argwhere(VM2).astype(np.int16)
    g["blocks_dims"] = np.array([len(Blocks), len(Blocks[0]), len(Blocks[0][0])])
    probe = [tuple(int(v) for v in out[3][i]) for i in (0, len(out[3]) // 2, len(out[3]) - 1)]
    g["blocks_probe"] = np.array(probe)
    for i, (bx, by, bz) in enumerate(probe):
        b = Blocks[bx][by][bz]
        assert b[0] is True and b[1].dtype == np.int8 and b[1].shape == (64, 64, 64) and len(b) == 4
        g["block%d_occ" % i] = np.argwhere(b[1]).astype(np.int16)
        g["block%d_local" % i] = np.array(b[2], np.int16); g["block%d_global" % i] = np.array(b[3], np.int16)
    empty = next((x, y, z) for x in range(len(Blocks)) for y in range(len(Blocks[0])) for z in range(len(Blocks[0][0]))
                 if Blocks[x][y][z][0] is False)
    assert Blocks[empty[0]][empty[1]][empty[2]] == [False]
    g["blocks_empty_probe"] = np.array(empty)
    np.savez_compressed(os.path.join(GOLD, "voxel_blocks.npz"), **g)
    print("  blocks golden: %d blocks, %d voxels" % (len(out[3]), len(out[6])))


def mat_golden():
    """the .mat stage files.  (1) WRITTEN BY THE REFERENCE -- its own functions / statements
    (BatchPreprocess.py:54-64 and :139-148, BatchVoxelization.BatchVoxelization :42-62, PoseEstimation.py:293-295 and
    :297-309) run on a small synthetic sequence -- and read back here with caelo.stageio (asserted equal); the files
    themselves are committed as the fixture tests/golden/mat_stage_files.npz so the CPU tests re-read them without the
    reference.  (2) WRITTEN BY caelo.stageio and read by the reference's own loaders (Match.LoadVoxelModelAndKeyPts,
    Match.LoadKeyPtsAndFeatures, Match.LoadVoxelModel, SphericalRing.GetKeyPtsFromRawFileName), asserted equal."""
    import shutil
    import tempfile
    from scipy import io
    import BatchVoxelization as RefBV
    from caelo import stageio
    tmp = tempfile.mkdtemp(prefix="caelo_mat_")
    g = {}
    try:
        seq = os.path.join(tmp, "ref", "00")
        os.makedirs(os.path.join(seq, "velodyne"))
        params = (0, 64, 1000)          # 64 beams x 1000 azimuths: ~63 k points, a few hundred key points, small files
        raws, clouds = [], []
        for f in (0, 1):
            pc = synth.make_scan(f, n_beams=params[1], n_az=params[2])
            raw = os.path.join(seq, "velodyne", "%06d.bin" % f)
            pc.tofile(raw)
            raws.append(raw); clouds.append(pc)
        g["scan_params"] = np.array(params); g["cloud_sha256"] = np.array([synth.cloud_sha256(c) for c in clouds])
        # ---- (1) the reference writes
        ring_block = ref_source_block(os.path.join(REF, "BatchPreprocess.py"), 54, 64)        # Projection + savemat
        keypt_block = ref_source_block(os.path.join(REF, "BatchPreprocess.py"), 136, 148)     # GetKeyPtsByAE .. savemat
        feat_block = ref_source_block(os.path.join(REF, "PoseEstimation.py"), 292, 295)       # for iFrame ...: savemat
        inl_block = ref_source_block(os.path.join(REF, "PoseEstimation.py"), 297, 309)
        frames = []
        for f, (raw, pc) in enumerate(zip(raws, clouds)):
            ns = {"np": np, "os": os, "io": io, "ProjectPC2SphericalRing": RefSR.ProjectPC2SphericalRing, "PC": pc,
                  "rawFileFullPath": raw, "TargetFolderName": "SphericalRing"}
            exec(ring_block, ns)
            ring, cnt = ns["SphericalRing"], ns["GridCounter"]
            resp = np.squeeze(resp_model.predict(ring[0:64, 0:1792, :][:, :, [0, 1, 2]].reshape(1, 64, 1792, 3)))
            ring_b = np.ascontiguousarray(ring[0:64, 0:1792, :][:, :, [0, 1, 2]]); cnt_b = np.array(cnt, dtype=np.int8)   # batch mode
            ns = {"np": np, "os": os, "io": io, "print": lambda *a, **k: None, "GetKeyPtsByAE": lambda *a: quiet(RefSR.GetKeyPtsByAE, *a)[0],
                  "ExtendKeyPtsInShpericalRing": RefSR.ExtendKeyPtsInShpericalRing, "SphericalRing": ring_b,
                  # the full int8 counter, as BatchPreprocess.py:98,132 hands it over
                  "GridCounter": cnt_b.copy(), "RespondImg": resp, "strDataBaseDir": os.path.dirname(seq),
                  "strSequence": "00", "KeyPtFolderName": "KeyPts", "iFrame": f, "nFramesInSequence": 2}
            exec(keypt_block, ns)
            kp, ext = ns["KeyPts"], ns["ExtendedKeyPts"]
            vout = RefVoxel.Voxelization(pc[:, 0:3])
            _, plist = RefVoxel.GetPatchesList(kp, vout[6], vout[7], vout[8])
            feats = RefMatch.GetFeaturesFromPatches(enc_model, plist)
            frames.append(dict(ring=ring, cnt=cnt, kp=kp, ext=ext, vout=vout, feats=feats, W=np.ones((len(kp), 1), np.float32)))
        quiet(RefBV.BatchVoxelization, raws, 0, [0])
        np.random.seed(5)
        (R, T, ok, i0, i1, thr), _ = quiet(RefMatch.SolveRelativePose, frames[0]["kp"], frames[0]["feats"], frames[0]["W"],
                                           frames[1]["kp"], frames[1]["feats"], frames[1]["W"])
        ns = {"os": os, "io": io, "str": str, "range": range, "len": len, "nFrames": 2, "FeatruesDataDir": os.path.join(seq, "Features"),
              "listKeyPtsData": [(fr["kp"], fr["feats"], fr["W"]) for fr in frames]}
        os.makedirs(ns["FeatruesDataDir"])
        exec(feat_block, ns)
        ns = {"os": os, "io": io, "strDataBaseDir": os.path.dirname(seq), "strSequence": "00", "iKeyPtSource": 0,
              "inliersData": [[0, 1, i0, i1]]}
        exec(inl_block, ns)
        # ... and caelo.stageio reads them back
        files = {}
        for f, (raw, fr) in enumerate(zip(raws, frames)):
            ring, cnt = stageio.load_spherical_ring(raw)
            assert ring.dtype == np.float32 and np.array_equal(ring, fr["ring"]) and np.array_equal(cnt, fr["cnt"])
            kp, a0, a1, a2 = stageio.load_voxel_model_and_keypts(raw)
            assert np.array_equal(kp, fr["kp"]) and np.array_equal(a0, fr["vout"][6]) and np.array_equal(a1, fr["vout"][7]) and np.array_equal(a2, fr["vout"][8])
            m = io.loadmat(stageio.mat_path(raw, "VoxelModel"))
            avl, cntl, local = stageio.block_structures(a0)
            assert np.array_equal(m["avlBlocksList"], avl) and np.array_equal(m["cntVoxelsLength"].ravel(), cntl) and np.array_equal(m["AllVoxels"], local)
            k2, F, W = stageio.load_keypts_and_features(raw)
            assert np.array_equal(k2, fr["kp"]) and np.array_equal(F, fr["feats"]) and np.array_equal(W, fr["W"])
            ke = io.loadmat(stageio.mat_path(raw, "KeyPts"))
            assert np.array_equal(ke["ExtendedKeyPts"], fr["ext"])
            g["f%d_ring_sha256" % f] = sha(fr["ring"]); g["f%d_counter_sha256" % f] = sha(fr["cnt"])
            g["f%d_keypts" % f] = fr["kp"]; g["f%d_ext_sha256" % f] = sha(np.asarray(fr["ext"], np.float32)); g["f%d_n_ext" % f] = len(fr["ext"])
            g["f%d_features" % f] = fr["feats"].astype(np.float32)
            g["f%d_voxel_sha256" % f] = np.array([sha(fr["vout"][6]), sha(fr["vout"][7]), sha(fr["vout"][8])])
            for folder in ("SphericalRing", "KeyPts", "VoxelModel", "Features"):
                if f == 1 and folder != "KeyPts":
                    continue            # the fixture keeps frame 0's five files, frame 1's KeyPts and the pair's InliersIdx
                with open(stageio.mat_path(raw, folder), "rb") as fh:
                    files["%s/%06d.bin.mat" % (folder, f)] = np.frombuffer(fh.read(), np.uint8)
        j0, j1 = stageio.load_inliers(seq, 0, 1)
        assert np.array_equal(j0, i0) and np.array_equal(j1, i1)
        with open(os.path.join(seq, "InliersIdx", "000000-000001.bin.mat"), "rb") as fh:
            files["InliersIdx/000000-000001.bin.mat"] = np.frombuffer(fh.read(), np.uint8)
        g["inliers_idx0"], g["inliers_idx1"] = i0.astype(np.int32), i1.astype(np.int32)
        g["file_names"] = np.array(sorted(files))
        for i, name in enumerate(sorted(files)):
            g["file_%d" % i] = files[name]
        # ---- (2) caelo.stageio writes, the reference's loaders read
        seq2 = os.path.join(tmp, "ours", "00")
        os.makedirs(os.path.join(seq2, "velodyne"))
        for f, fr in enumerate(frames):
            raw = os.path.join(seq2, "velodyne", "%06d.bin" % f)
            stageio.save_spherical_ring(raw, fr["ring"], fr["cnt"])
            stageio.save_keypts(raw, fr["kp"], fr["ext"])
            stageio.save_voxel_model(raw, fr["vout"][6], fr["vout"][7], fr["vout"][8])
            stageio.save_features(raw, fr["kp"], fr["feats"])
            kp, a0, a1, a2 = RefMatch.LoadVoxelModelAndKeyPts(raw)
            assert np.array_equal(kp, fr["kp"]) and np.array_equal(a0, fr["vout"][6]) and np.array_equal(a1, fr["vout"][7]) and np.array_equal(a2, fr["vout"][8])
            k2, F, W = RefMatch.LoadKeyPtsAndFeatures(raw)
            assert np.array_equal(k2, fr["kp"]) and np.array_equal(F, fr["feats"]) and np.array_equal(W, fr["W"])
            Blocks, VM1, VM2 = RefMatch.LoadVoxelModel(raw)          # rebuilds the voxel models from OUR block structures
            assert np.array_equal(VM1, fr["vout"][1]) and np.array_equal(VM2, fr["vout"][2])
            for bx, by, bz in fr["vout"][3][:: max(1, len(fr["vout"][3]) // 7)]:
                assert np.array_equal(Blocks[bx][by][bz][1], fr["vout"][0][bx][by][bz][1])
            (kp3, kpix3, _), _ = quiet(RefSR.GetKeyPtsFromRawFileName, raw, resp_model)      # demo mode on OUR ring file
            (kp4, kpix4, _), _ = quiet(RefSR.GetKeyPtsFromRawFileName, raws[f], resp_model)   # ... and on the reference's
            assert np.array_equal(kp3, kp4) and np.array_equal(kpix3, kpix4)
            g["f%d_keypixels_from_raw" % f] = kpix4.astype(np.int16); g["f%d_keypts_from_raw" % f] = kp4.astype(np.float32)
        stageio.save_inliers(seq2, 0, 1, i0, i1)
        m = io.loadmat(os.path.join(seq2, "InliersIdx", "000000-000001.bin.mat"))
        assert np.array_equal(m["inliersIdx0"].ravel(), i0) and int(m["iFrame1"]) == 1
        g["reference_loaders_read_stageio_files"] = True
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(GOLD, "mat_stage_files.npz"), **g)
    print("  mat golden: %d reference-written files (%.0f KB raw), K = %d / %d, %d inliers" % (
        len(files), sum(v.size for v in files.values()) / 1024, len(frames[0]["kp"]), len(frames[1]["kp"]), len(i0)))


def ref_source_block(path, first, last):
    """Lines first..last (1-based, inclusive) of a reference script, dedented -- for the statements of
    PoseEstimation.py's __main__ that are not inside a function and therefore cannot be imported."""
    import textwrap
    with open(path) as f:
        lines = f.read().split("\n")[first - 1:last]
    return textwrap.dedent("\n".join(lines))


def sequence_golden(n_frames=20, seed_base=1000):
    """SURVEY 8c harness row: per-pair (R, T, nInliers, thr) of consecutive synthetic frames through the reference's
    own functions (PoseEstimation.py:152-167 = SolveRelativePose on the stored KeyPts / Features), RANSAC seeded
    per pair with np.random.seed(seed_base + iFrame0), and the pose chaining statements of PoseEstimation.py
    (:202-207 calibration, :232 first pose, :253-267 update) EXECUTED from the reference source, once with Tr = I and
    once with a KITTI-like Tr.  The oracle is asserted against every pair."""
    import Transformations as RefT
    t0 = time.time()
    frames = []
    for f in range(n_frames):
        pc = synth.make_scan(f)
        ring, cnt = RefSR.ProjectPC2SphericalRing(pc)
        resp = np.squeeze(resp_model.predict(ring[0:64, 0:1792, :][:, :, [0, 1, 2]].reshape(1, 64, 1792, 3)))
        (kp, kpix, _), _ = quiet(RefSR.GetKeyPtsByAE, ring, cnt, resp)
        vout = RefVoxel.Voxelization(pc[:, 0:3])
        _, plist = RefVoxel.GetPatchesList(kp, vout[6], vout[7], vout[8])
        feats = RefMatch.GetFeaturesFromPatches(enc_model, plist)
        frames.append((kp, feats))
        print("  seq frame %d: K=%d (%.0fs)" % (f, len(kp), time.time() - t0))
    g = {"n_frames": n_frames, "seed_base": seed_base}
    rel = np.zeros((n_frames - 1, 12), np.float32)
    nin = np.zeros(n_frames - 1, np.int32); thr = np.zeros(n_frames - 1, np.float32); ok = np.zeros(n_frames - 1, bool)
    for i in range(n_frames - 1):
        (kp0, F0), (kp1, F1) = frames[i], frames[i + 1]
        W0 = np.ones((len(kp0), 1), np.float32); W1 = np.ones((len(kp1), 1), np.float32)
        np.random.seed(seed_base + i)
        (R, T, isok, i0, i1, th), _ = quiet(RefMatch.SolveRelativePose, kp0, F0, W0, kp1, F1, W1)
        oR, oT, ook, oi0, oi1, oth = orc.SolveRelativePose(kp0, F0, W0, kp1, F1, W1, rng=np.random.RandomState(seed_base + i))
        assert ook == isok and oth == th and np.array_equal(oi0, i0) and np.allclose(oR, R, atol=1e-6) and np.allclose(oT, T, atol=1e-5)
        assert R.dtype == np.float32 and np.asarray(T).dtype == np.float32
        rel[i, :9] = np.asarray(R).ravel(); rel[i, 9:] = np.asarray(T).ravel()
        nin[i], thr[i], ok[i] = len(i0), th, isok
        print("  seq pair %d-%d: ok=%s thr=%.1f inliers=%d T=%s" % (i, i + 1, isok, th, len(i0), np.round(np.asarray(T).ravel(), 3)))
    g.update(rel_rt=rel, n_inliers=nin, threshold=thr, success=ok, n_key=np.array([len(k) for k, _ in frames], np.int32))
    calib_block = ref_source_block(os.path.join(REF, "PoseEstimation.py"), 203, 207)   # Tr -> R_Tr, R_Tr_inv, T_Tr, T_Tr_inv
    chain_block = ref_source_block(os.path.join(REF, "PoseEstimation.py"), 253, 267)   # pose0 -> pose1
    kitti_tr = np.array([4.276802385584e-04, -9.999672484946e-01, -8.084491683471e-03, -1.198459927713e-02,
                         -7.210626507497e-03, 8.081198471645e-03, -9.999413164504e-01, -5.403984729748e-02,
                         9.999738645903e-01, 4.859485810390e-04, -7.206933692422e-03, -2.921968648686e-01])
    for name, tr in (("identity", np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)), ("kitti", kitti_tr)):
        ns = {"np": np, "GetRtFromOnePose": RefT.GetRtFromOnePose, "calib": np.tile(tr, (5, 1))}
        exec(calib_block, ns)
        ns["poses"] = [np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32).reshape(12, 1)]   # :231-233
        for i in range(n_frames - 1):
            ns.update(iFrame0=i, relativeR=rel[i, :9].reshape(3, 3), relativeT=rel[i, 9:].reshape(3, 1))
            exec(chain_block, ns)
        poses = np.array(ns["poses"], dtype=np.float32)
        g["poses_" + name] = poses.reshape(poses.shape[0], 12)                                             # :273-274
        g["tr_" + name] = tr
        print("  seq poses (%s): last T = %s" % (name, np.round(g["poses_" + name][-1].reshape(3, 4)[:, 3], 3)))
    np.savez_compressed(os.path.join(GOLD, "sequence_20.npz"), **g)


if __name__ == "__main__":
    t0 = time.time()
    if "--sequence-only" in sys.argv:
        sequence_golden()
        sys.exit(0)
    if "--trunc-only" in sys.argv:
        trunc_golden()
        tie_golden()
        sys.exit(0)
    if "--brute-only" in sys.argv:
        brute_golden()
        sys.exit(0)
    if "--shuffled-only" in sys.argv:
        shuffled_golden()
        sys.exit(0)
    if "--clutter-only" in sys.argv:
        clutter_golden()
        sys.exit(0)
    if "--quantised-only" in sys.argv:
        quantised_golden()
        sys.exit(0)
    if "--refine-only" in sys.argv:
        refine_golden()
        sys.exit(0)
    if "--mat-only" in sys.argv:
        mat_golden()
        sys.exit(0)
    if "--blocks-only" in sys.argv:
        blocks_golden()
        sys.exit(0)
    if "--extend-only" in sys.argv:
        extend_golden()
        sys.exit(0)
    if "--icp-only" in sys.argv:
        icp_golden()
        icp_loop_golden()
        sys.exit(0)
    trunc_golden()
    brute_golden()
    f0 = frame_golden(0)
    f1 = frame_golden(1)
    pair_golden(f0, f1)
    quantised_golden()
    clutter_golden()
    tie_golden()
    shuffled_golden()
    # dense 128-beam scan: exercises the 496-NN truncation of GetPatchesList
    frame_golden(0, n_beams=128, n_az=4000, n_patch_kp=192, tag="dense128")
    sequence_golden()
    blocks_golden()
    mat_golden()
    extend_golden()
    icp_golden()
    icp_loop_golden()
    refine_golden()
    print("done in %.1fs" % (time.time() - t0))
    for f in sorted(os.listdir(GOLD)):
        print("  %-24s %8.1f KB" % (f, os.path.getsize(os.path.join(GOLD, f)) / 1024))
