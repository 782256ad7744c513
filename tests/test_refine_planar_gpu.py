"""refine_sequence.py --icp pt2plane --planar-pts ring end to end on the device: 8 synthetic frames through run_sequence.py with the
artefacts kept, then the refinement with every frame's planar points made by caelo_planar_points -- under --nn grid and --nn brute,
again from the KeyPts files the first run saved, and the same walk on the host with the oracle's ICP_Pt2PtAndPt2Plane fed the same
extended and planar sets and the same subsample seeds.

Bars on the poses: four times the differences measured against the oracle walk (profiles/planar_errors.txt: max |dR| 3.2e-07, max |dT|
3.2e-05 m), the project's convention for float32 fits inside an ICP."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

SEED_BASE = 1034
BAR_R, BAR_T = 4 * 3.2e-07, 4 * 3.2e-05
# The oracle's smallest |distance - threshold| over every gate of every iteration must not be marginal.  The device keeps the moved
# frame 1 in float32, so a distance nearer to its threshold than one float32 step of a coordinate (3.8e-6 m from 32 m on; the scans
# reach 64 m) may fall either way.  SEED_BASE -- the subsample of the 5 370 planar points of frame 6 -- is chosen for it: 1.4e-5 m.
MIN_MARGIN = 4e-6


def _tree_neighbours(PC0, PC1, chunk=None):
    """oracle.nearest_neighbours (exact float64 distances, brute force) through a kd-tree, as tests/test_refine_sequence_gpu.py does:
    an extended set holds 10^5 points.  The test asserts equal indices and distances on its two smallest sets."""
    from scipy.spatial import cKDTree
    d, i = cKDTree(np.asarray(PC0, np.float64)).query(np.asarray(PC1, np.float64), k=1, workers=-1)
    return d, i.astype(np.int64)


def test_pt2plane_from_ring_planar_points(engine, orc, tmp_path, monkeypatch):
    from scipy import io
    import refine_sequence
    from caelo import refine, stageio
    out = str(tmp_path / "poses_" / "00.txt")
    subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "run_sequence.py"), "--synthetic", "8", "--save-artifacts", "--out", out],
                   check=True, capture_output=True, timeout=300)
    seq = os.path.join(os.path.dirname(out), "synthetic")
    common = ["--poses", out, "--inliers-dir", os.path.join(seq, "InliersIdx"), "--mode", "keyframes", "--icp", "pt2plane", "--seed-base", str(SEED_BASE)]
    runs = {}
    for nn in ("grid", "brute"):
        runs[nn] = refine_sequence.run(common + ["--synthetic", "--planar-pts", "ring", "--nn", nn, "--out", str(tmp_path / nn / "poses___.txt"),
                                                 "--save-keypts", os.path.join(seq, "KeyPts_" + nn)])
    r = runs["grid"]
    assert (tmp_path / "grid" / "poses___.txt").read_bytes() == (tmp_path / "brute" / "poses___.txt").read_bytes()
    assert (r["tried"], r["failed"]) == (runs["brute"]["tried"], runs["brute"]["failed"])
    assert any(t[2] == 1 for t in r["tried"]) and np.isfinite(r["poses"]).all()

    # the files the run saved: every frame it used, with its planar points; a run from them writes the same poses
    used = sorted({f for t in r["tried"] for f in t[:2]})
    ext, planar = {}, {}
    for f in used:
        m = io.loadmat(os.path.join(seq, "KeyPts_grid", "%06d.bin.mat" % f))
        b = io.loadmat(os.path.join(seq, "KeyPts_brute", "%06d.bin.mat" % f))
        ext[f], planar[f] = np.ascontiguousarray(m["ExtendedKeyPts"], dtype=np.float32), np.ascontiguousarray(m["PlanarPts"], dtype=np.float32)
        assert planar[f].ndim == 2 and planar[f].shape[1] == 6 and planar[f].shape[0] > 2000 and (planar[f][:, 5] > 0.9).all()
        assert planar[f].tobytes() == np.ascontiguousarray(b["PlanarPts"], dtype=np.float32).tobytes()
    rest = refine_sequence.KeyPts(engine, 8, synthetic=dict(scene_kind="boxes", trajectory="circuit"), save_dir=os.path.join(seq, "KeyPts_grid"), planar_ring=True)
    for f in set(range(8)) - set(used):   # (--keypts-dir wants a file for every frame of the pose file: the tool's own maker writes the rest)
        assert rest(f)[1].shape[0] > 2000
    again = refine_sequence.run(common + ["--keypts-dir", os.path.join(seq, "KeyPts_grid"), "--nn", "grid", "--out", str(tmp_path / "files" / "poses___.txt")])
    assert again["tried"] == r["tried"]
    assert (tmp_path / "files" / "poses___.txt").read_bytes() == (tmp_path / "grid" / "poses___.txt").read_bytes()

    # the host walk: RefinementCore as it is, the oracle's ICP_Pt2PtAndPt2Plane on the same sets, the k-th call with RandomState(SEED_BASE + k)
    a, b = sorted(ext.values(), key=lambda x: x.shape[0])[:2]   # the kd-tree substitution itself, on the two smallest sets: the same neighbours
    d_brute, i_brute = orc.nearest_neighbours(a, b)
    d_tree, i_tree = _tree_neighbours(a, b)
    assert np.array_equal(i_brute, i_tree) and np.array_equal(d_brute, d_tree)
    monkeypatch.setattr(orc, "nearest_neighbours", _tree_neighbours)
    margins, pairs = [], []

    def icp(*args, **kw):
        steps = []
        res = orc.ICP_Pt2PtAndPt2Plane(*args, steps=steps, **kw)
        margins.append(min(s["margin"] for s in steps))
        pairs.append((steps[0]["n_pts"], steps[0]["n_planar"]))
        return res
    core = refine.make_core(lambda f: (ext[f], planar[f]), np.eye(3, 4, dtype=np.float32), icp, seed_base=SEED_BASE)
    host, info, failed, tried = refine.RefineOdometry(np.loadtxt(out).reshape(-1, 12), 1, core, pairs=lambda f0, f1: stageio.load_inliers(seq, f0, f1))
    got, want = r["poses"].reshape(-1, 3, 4), host.reshape(-1, 3, 4)
    dR, dT = np.abs(got[:, :, :3] - want[:, :, :3]).max(), np.abs(got[:, :, 3] - want[:, :, 3]).max()
    print("refine_planar_gpu: n_ext %s, n_planar %s, pairs %s, first-iteration (point, planar) pairs %s, smallest gate margin %.3e, max |dR| %.3e, max |dT| %.3e"
          % ([ext[f].shape[0] for f in used], [planar[f].shape[0] for f in used], r["tried"], pairs, min(margins), dR, dT))
    assert min(margins) > MIN_MARGIN
    assert (tried, failed) == (r["tried"], r["failed"])
    assert np.array_equal(info[:, 0:2], r["debug"][:, 0:2])
    assert dR <= BAR_R and dT <= BAR_T
