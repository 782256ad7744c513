"""The device pass of the key point evaluation (caelo_kp_nn_pairs, csrc/evaluate.hip) against scikit-learn 0.24.2's kd-tree distances
recorded from the reference (tests/golden/evaluate.npz), a float64 NumPy restatement, and end to end through run_sequence.py and
evaluate.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import io

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))

from caelo import evaluate as ev  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden", "evaluate.npz")
STEPS = (1, 2, 10)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def eng():
    from caelo.engine import Engine
    return Engine(respond_h5=None, encoder_h5=None)


def golden_lists(g, src, step):
    """Per sequence: the golden world-frame key points of every step-th frame (the reference's GetAllKeyPts output)."""
    nfr = g["n_frames"]
    fo = np.r_[0, np.cumsum(nfr)]
    po = np.r_[0, np.cumsum(g["kp_count_" + src])]
    w = g["world_" + src]
    return [[w[po[f]:po[f + 1]] for f in range(fo[s], fo[s + 1])][::step] for s in range(len(nfr))]


@pytest.mark.parametrize("src", ev.SOURCES)
@pytest.mark.parametrize("step", STEPS)
def test_device_distances_equal_reference_kdtree_bitwise(g, eng, src, step):
    """Every K of the golden (4, 5, 6-27, 1100, 1500: beyond one LDS chunk), float32 and float64 world points, repeated
    coordinates and a repeated frame: the distances are the reference's bits and the counts its script's, in both modes (mode 1:
    every pair is (k, k) and every distance 0)."""
    si, sti = ev.SOURCES.index(src), STEPS.index(step)
    for mode in (0, 1):
        ds, pos = g["dist%d_%s_%d" % (mode, src, step)], 0
        for s, lst in enumerate(golden_lists(g, src, step)):
            d, c = ev.device_distances(lst, inner=bool(mode), engine=eng)
            ref = ds[pos:pos + d.shape[0]]
            pos += d.shape[0]
            assert d.dtype == np.float64 and d.shape == (ref.shape[0], 1)
            assert np.array_equal(d.ravel().view(np.uint64), ref.view(np.uint64)), "seq %d mode %d: %d distances differ" % (
                s, mode, int((d.ravel() != ref).sum()))
            assert c.tolist() == g["counts"][mode, sti, si, s].tolist()
        assert pos == ds.shape[0]
        if mode == 1:
            assert not ds.any()
    if step == 1:
        ks = {a.shape[0] for lst in golden_lists(g, src, 1) for a in lst}
        assert {4, 5, 1100, 1500} <= ks


def test_boundary_distances_and_bins(g, eng):
    """Distances exactly at D_t, one ulp below and one above, per threshold: D_t itself falls in the next bin (dist / D_t < 1 is
    false), so a kernel that compared dist <= D_t would count differently."""
    pts = np.zeros((2, g["boundary_query"].shape[0], 3))
    pts[0, :5] = g["boundary_fit"]
    pts[1] = g["boundary_query"]
    dist, counts = eng.kp_nn_pairs(pts, [5, pts.shape[1]], [[0, 1]], ev.DISCRETIZATIONS)
    d = dist.cpu().numpy()[0]
    assert np.array_equal(d.view(np.uint64), g["boundary_dist"].view(np.uint64))
    assert counts.cpu().numpy()[0].tolist() == g["boundary_counts"].tolist()
    le = [int(np.sum(d <= D)) for D in ev.DISCRETIZATIONS]
    assert np.diff([0] + le).tolist() != counts.cpu().numpy()[0][:-1].tolist()


def brute(fit, query):
    """scikit-learn's euclidean_rdist restated in float64 NumPy (every operation rounded on its own, x, y, z in order), the minimum,
    then sqrt."""
    dx = query[:, None, 0] - fit[None, :, 0]
    dy = query[:, None, 1] - fit[None, :, 1]
    dz = query[:, None, 2] - fit[None, :, 2]
    r = dx * dx
    r = r + dy * dy
    r = r + dz * dz
    return np.sqrt(r.min(axis=1))


def test_device_distances_equal_numpy_restatement(eng):
    rng = np.random.default_rng(1234)
    ks = [4, 5, 64, 255, 257, 1024, 1025, 1500, 3000]
    sets = []
    for k in ks:
        a = rng.uniform(-50, 50, (k, 3))
        a[rng.integers(0, k, k // 4)] = a[rng.integers(0, k, k // 4)]   # duplicated points
        a[:, 2] = np.round(a[:, 2], 1)                                    # repeated coordinates
        sets.append(a)
    sets.append(sets[3].copy())                                           # a frame that repeats a whole set
    sets[4][:100] = sets[5][:100] + 1e-9
    pairs = [(i, j) for i in range(len(sets)) for j in (i - 1, i, i + 1) if 0 <= j < len(sets)]
    pts, nk = ev.stack_keypts(sets)
    dist, counts = eng.kp_nn_pairs(pts, nk, pairs, ev.DISCRETIZATIONS)
    dist, counts = dist.cpu().numpy(), counts.cpu().numpy()
    for p, (i, j) in enumerate(pairs):
        ref = brute(sets[i], sets[j])
        assert np.array_equal(dist[p, :nk[j]].view(np.uint64), ref.view(np.uint64)), (i, j)
        assert np.isnan(dist[p, nk[j]:]).all()
        assert counts[p].tolist() == [int(c) for c in ev.RepeatabilityCounts(ref.reshape(-1, 1))]
        if i == j:
            assert not ref.any()


def test_device_refuses_before_launch(eng):
    pts = np.random.default_rng(0).uniform(-1, 1, (2, 8, 3))
    with pytest.raises(ValueError, match="3 points or fewer"):
        eng.kp_nn_pairs(pts, [3, 8], [[0, 1]], ev.DISCRETIZATIONS)
    bad = pts.copy(); bad[1, 2, 0] = np.inf
    with pytest.raises(ValueError, match="NaN, infinity"):
        eng.kp_nn_pairs(bad, [8, 8], [[0, 1]], ev.DISCRETIZATIONS)
    bad[1, 2, 0] = 0.0; bad[1, 7, 0] = np.nan   # past n_key: not part of the set
    eng.kp_nn_pairs(bad, [8, 7], [[0, 1]], ev.DISCRETIZATIONS)
    with pytest.raises(ValueError, match="outside"):
        eng.kp_nn_pairs(pts, [8, 8], [[0, 2]], ev.DISCRETIZATIONS)
    with pytest.raises(ValueError, match="thresholds"):
        eng.kp_nn_pairs(pts, [8, 8], [[0, 1]], [0.1, float("nan")])
    torch.cuda.synchronize()


def test_end_to_end_run_sequence_and_evaluate(tmp_path, eng):
    """run_sequence.py --synthetic 40 --save-artifacts --matchability, then both evaluate.py subcommands: their files equal the
    Python API on the same files, and the measured figures are pinned."""
    from caelo import synth
    import math
    out = tmp_path / "poses_" / "00.txt"
    m = tmp_path / "Matchablity_1_0-0_00.mat"
    rs = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
    evp = os.path.join(REPO, "cae-lo_amd", "evaluate.py")
    subprocess.run([sys.executable, rs, "--synthetic", "40", "--trajectory", "circuit", "--save-artifacts", "--matchability", str(m),
                    "--out", str(out)], check=True, capture_output=True, timeout=900)
    n = 40
    gt = np.zeros((n, 12))
    for i in range(n):
        (x, y, z), yaw = synth.sensor_pose(i, trajectory="circuit")
        c, s = math.cos(yaw), math.sin(yaw)
        gt[i] = np.array([[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, z]]).reshape(12)
    gtp = tmp_path / "gt.txt"
    np.savetxt(str(gtp), gt)
    calib = tmp_path / "calib_.txt"
    cm = np.zeros((5, 12)); cm[4] = np.eye(3, 4).reshape(12)
    np.savetxt(str(calib), cm)
    prop, trials = ev.load_matchability(str(m))
    assert prop.shape == (1, n - 1) and trials.shape == (1, n - 1)

    reg = tmp_path / "EvaluationResults.mat"
    r = subprocess.run([sys.executable, evp, "registration", "--gt", str(gtp), "--est", str(out), "--calib", str(calib),
                        "--matchability", str(m), "--out", str(reg)], check=True, capture_output=True, text=True, timeout=300)
    row_file = io.loadmat(str(reg))["EvaluationResults"]
    row, ok = ev.registration([str(gtp)], [str(out)], [str(calib)], [str(m)])
    assert row_file.shape == (1, 7) and row_file.dtype == np.float32 and np.array_equal(row_file[0], row)

    feats = tmp_path / "poses_" / "synthetic" / "Features"
    kp = tmp_path / "AccuracyOfKeyPts_1_0_00.mat"
    subprocess.run([sys.executable, evp, "keypoints", "--keypts-dir", str(feats), "--source", "ae", "--gt", str(gtp), "--calib", str(calib),
                    "--out", str(kp)], check=True, capture_output=True, text=True, timeout=300)
    counts_file = io.loadmat(str(kp))["counts"]
    counts, d = ev.repeatability(str(feats), "ae", np.loadtxt(str(gtp)), ev.read_tr(str(calib)), engine=eng)
    assert counts_file.shape == (1, 8) and counts_file.ravel().tolist() == [int(c) for c in counts]
    print("registration row", row.tolist(), "successes", int(ok.sum()), "of", ok.shape[0], r.stdout.strip())
    print("repeatability counts", [int(c) for c in counts], "over", d.shape[0], "points")
    assert int(ok.sum()) == PINNED_SUCCESSES and [int(c) for c in counts] == PINNED_COUNTS


# measured on MI355X: 37 of the 39 pairs register (RRE < 1 deg and RTE < 0.5 m); the two that do not are the engine's
# RANSAC results on this synthetic circuit, reported as they are
PINNED_SUCCESSES = 37
PINNED_COUNTS = [5104, 3499, 7257, 7983, 13417, 1805, 678, 193]
