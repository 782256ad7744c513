"""refine_sequence.py end to end on the device: 8 synthetic frames through run_sequence.py with the artefacts kept, a jump planted
into the pose file, then --dejump --mode keyframes under --nn grid and --nn brute, and the same walk on the host with the oracle's
ICP on the same extended key point sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

JUMP_FRAME, JUMP_M = 4, 2.0   # four times FixJumpPoses' 0.5 m


def _tree_neighbours(PC0, PC1, chunk=None):
    """oracle.nearest_neighbours (exact float64 distances, brute force) through a kd-tree: an extended set holds 10^5 points, which
    the brute force does not finish in a test's time.  The test asserts equal indices and distances on its two smallest sets."""
    from scipy.spatial import cKDTree
    d, i = cKDTree(np.asarray(PC0, np.float64)).query(np.asarray(PC1, np.float64), k=1, workers=-1)
    return d, i.astype(np.int64)


def test_grid_and_brute_write_the_same_files_and_follow_the_host_walk(engine, orc, tmp_path, monkeypatch):
    from scipy import io
    import refine_sequence
    from caelo import refine
    out = str(tmp_path / "poses_" / "00.txt")
    subprocess.run([sys.executable, os.path.join(REPO, "cae-lo_amd", "run_sequence.py"), "--synthetic", "8", "--save-artifacts", "--out", out],
                   check=True, capture_output=True, timeout=300)
    poses = np.loadtxt(out).reshape(-1, 12)
    assert poses.shape[0] == 8
    step = poses[JUMP_FRAME, [3, 7, 11]] - poses[JUMP_FRAME - 1, [3, 7, 11]]
    poses[JUMP_FRAME:, [3, 7, 11]] += JUMP_M * step / np.linalg.norm(step)   # the motion into JUMP_FRAME grows by 2 m; later motions stay
    jumped = str(tmp_path / "poses_" / "jump.txt")
    np.savetxt(jumped, poses)
    seq = os.path.join(os.path.dirname(out), "synthetic")
    runs = {}
    for nn in ("grid", "brute"):
        d = tmp_path / nn
        runs[nn] = refine_sequence.run(["--poses", jumped, "--inliers-dir", os.path.join(seq, "InliersIdx"), "--synthetic", "--dejump", "--mode", "keyframes",
                                        "--nn", nn, "--out", str(d / "poses___.txt"), "--dejumped-out", str(d / "poses__.txt"),
                                        "--debug-info", str(d / "DebugInfo.mat"), "--save-keypts", os.path.join(seq, "KeyPts_" + nn)])
    for name, skip in (("poses___.txt", 0), ("poses__.txt", 0), ("DebugInfo.mat", 128)):   # (a MAT-5 file opens with 128 bytes of header text: its creation time)
        assert (tmp_path / "grid" / name).read_bytes()[skip:] == (tmp_path / "brute" / name).read_bytes()[skip:], name
    r = runs["grid"]
    assert r["fixed"] == [JUMP_FRAME] and (r["tried"], r["failed"]) == (runs["brute"]["tried"], runs["brute"]["failed"])
    assert io.loadmat(str(tmp_path / "grid" / "DebugInfo.mat"))["aDebugInfo"].shape == (len([t for t in r["tried"] if t[2] == 1]), 4)
    assert any(t[2] == 1 for t in r["tried"]) and np.isfinite(r["poses"]).all()

    # the host walk: the same extended sets, RefinementCore as it is, the oracle's ICP (RefinePoses.py:295)
    sets = {f: np.ascontiguousarray(io.loadmat(os.path.join(seq, "KeyPts_grid", "%06d.bin.mat" % f))["ExtendedKeyPts"], dtype=np.float32)
            for f in {f for t in r["tried"] for f in t[:2]}}
    for f, a in sets.items():
        assert a.tobytes() == np.ascontiguousarray(io.loadmat(os.path.join(seq, "KeyPts_brute", "%06d.bin.mat" % f))["ExtendedKeyPts"], dtype=np.float32).tobytes()
    a, b = sorted(sets.values(), key=lambda x: x.shape[0])[:2]   # the substitution itself, on the two smallest sets: the same neighbours
    d_brute, i_brute = orc.nearest_neighbours(a, b)
    d_tree, i_tree = _tree_neighbours(a, b)
    assert np.array_equal(i_brute, i_tree) and np.array_equal(d_brute, d_tree)
    monkeypatch.setattr(orc, "nearest_neighbours", _tree_neighbours)
    from caelo import stageio
    core = refine.make_core(lambda f: (sets[f], np.zeros((0, 6), np.float32)), np.eye(3, 4, dtype=np.float32), refine.pt2pt_adapter(lambda a, b: orc.ICP(a, b)))
    dejumped, fixed = refine.FixJumpPoses(np.loadtxt(jumped).reshape(-1, 12))
    host, info, failed, tried = refine.RefineOdometry(dejumped, 1, core, pairs=lambda f0, f1: stageio.load_inliers(seq, f0, f1))
    assert (fixed, tried, failed) == (r["fixed"], r["tried"], r["failed"])
    assert np.array_equal(info[:, 0:2], r["debug"][:, 0:2])
    got, want = r["poses"].reshape(-1, 3, 4), host.reshape(-1, 3, 4)
    print("refine_sequence_gpu: n_ext %s, pairs %s, max |dR| %.3e, max |dT| %.3e" % (sorted(a.shape[0] for a in sets.values()), r["tried"],
          np.abs(got[:, :, :3] - want[:, :, :3]).max(), np.abs(got[:, :, 3] - want[:, :, 3]).max()))
    assert np.abs(got[:, :, :3] - want[:, :, :3]).max() <= 1e-4 and np.abs(got[:, :, 3] - want[:, :, 3]).max() <= 5e-4   # the ICP tests' tolerance
