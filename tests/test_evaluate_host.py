"""caelo.evaluate's host code against the reference's evaluation scripts (tests/golden/evaluate.npz, tools/make_goldens_evaluate.py).

The golden was made with NumPy 1.26 (the reference's dtype rules) and scikit-learn 0.24.2; this process may run NumPy 2.x with
another BLAS.  Values that go through BLAS (np.dot of the world transform and the pose algebra) may therefore differ by at most
2 ulp (MAX_ULP) of the largest magnitude that enters their sums: a world point by 2 ulp of the largest of its frame's world
coordinates and pose translation, a translation error by 2 ulp of twice the sequence's largest pose translation (T1 and
inv(R0) T0 of magnitude |T| each enter one sum: the errors are small differences of large terms), an Euler error or a registration row entry by 2 ulp of its row's largest entry.  Everything counted --
success flags, histogram counts, shapes and dtypes -- must be identical.
"""
import os
import sys

import numpy as np
import pytest
from scipy import io

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cae-lo_amd"))

from caelo import evaluate as ev, keysources  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluate.npz")
MAX_ULP = 2
STEPS = (1, 2, 10)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def close(a, b, scale=None):
    """|a - b| <= MAX_ULP ulp of ``scale`` (the largest magnitude that enters the sums; default: each row's largest entry)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    if scale is None:
        scale = np.abs(b).max(axis=-1, keepdims=True)
    ulp = np.spacing(np.asarray(scale, dtype=b.dtype)).astype(np.float64)
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert (d <= MAX_ULP * ulp).all(), "max deviation %.3g ulp of the scale" % (d / ulp).max()


def seq_slices(n_frames):
    off = np.r_[0, np.cumsum(n_frames)]
    return [slice(int(off[s]), int(off[s + 1])) for s in range(len(n_frames))]


@pytest.fixture(scope="module")
def tree(g, tmp_path_factory):
    """The golden's inputs written back as the reference's files: per sequence gt.txt, calib_.txt and the three key point folders."""
    root = tmp_path_factory.mktemp("eval_tree")
    nfr = g["n_frames"]
    frames = seq_slices(nfr)
    for src in ev.SOURCES:
        off = np.r_[0, np.cumsum(g["kp_count_" + src])]
        for s, sl in enumerate(frames):
            for i, f in enumerate(range(sl.start, sl.stop)):
                pts = g["kp_" + src][off[f]:off[f + 1]]
                d = root / ("%02d" % s) / src
                if src == "ae":
                    d.mkdir(parents=True, exist_ok=True)
                    io.savemat(str(d / ("%06d.bin.mat" % i)), {"KeyPts": pts})
                elif src == "3dfeatnet":
                    keysources.write_3dfeatnet(str(d / ("%06d.bin" % i)), pts)
                else:
                    keysources.write_usip(str(d / ("%06d.bin" % i)), pts)
    for s, sl in enumerate(frames):
        np.savetxt(str(root / ("%02d" % s) / "gt.txt"), g["gt_poses"][sl])
        calib = np.zeros((5, 12)); calib[4] = g["tr"][s].astype(np.float64).reshape(12)
        np.savetxt(str(root / ("%02d" % s) / "calib_.txt"), calib, fmt="%.17g")
    return root


@pytest.mark.parametrize("src", ev.SOURCES)
@pytest.mark.parametrize("step", STEPS)
def test_world_points_match_reference(g, tree, src, step):
    """GetAllKeyPts / TranslatePtsIntoWorldFrame: float32 for 'ae' and '3dfeatnet', float64 for 'usip' (R90), at frame steps 1, 2, 10."""
    frames = seq_slices(g["n_frames"])
    world = g["world_" + src]
    off = np.r_[0, np.cumsum(g["kp_count_" + src])]
    assert world.dtype == (np.float64 if src == "usip" else np.float32)
    for s, sl in enumerate(frames):
        d = tree / ("%02d" % s)
        pts = ev.GetAllKeyPts(str(d / src), src, np.loadtxt(str(d / "gt.txt")), ev.read_tr(str(d / "calib_.txt")), step)
        idx = list(range(sl.start, sl.stop))[::step]
        assert len(pts) == len(idx)
        for a, f in zip(pts, idx):
            ref = world[off[f]:off[f + 1]]
            close(a, ref, max(np.abs(ref).max(), np.abs(g["gt_poses"][f].reshape(3, 4)[:, 3]).max()))


def _ref_dists(g, src, step, mode):
    return g["dist%d_%s_%d" % (mode, src, step)]


@pytest.mark.parametrize("src", ev.SOURCES)
@pytest.mark.parametrize("step", STEPS)
def test_repeatability_counts_on_reference_distances(g, src, step):
    """The histogram loop (EvaluationOnKeypts.py:128-140) over the reference's own distances gives the counts its script wrote --
    per sequence; mode 1's distances are all 0, so all its counts sit in the first bin."""
    si = ev.SOURCES.index(src)
    counts = g["counts"]   # [mode, step, source, seq, T+1]
    frames = seq_slices(g["n_frames"])
    off = np.r_[0, np.cumsum(g["kp_count_" + src])]
    si_step = STEPS.index(step)
    for mode in (0, 1):
        d = _ref_dists(g, src, step, mode)
        pos = 0
        for s, sl in enumerate(frames):
            idx = list(range(sl.start, sl.stop))[::step]
            q = idx[1:] if mode == 0 else idx
            n = int(sum(off[f + 1] - off[f] for f in q))
            mine = ev.RepeatabilityCounts(d[pos:pos + n].reshape(-1, 1))
            pos += n
            assert [int(c) for c in mine] == counts[mode, si_step, si, s].tolist()
        assert pos == d.shape[0]
        if mode == 1:
            assert not d.any() and (counts[1, si_step, si, :, 1:] == 0).all()


def test_boundary_distances_bin_with_ieee_division(g):
    """Query points at exactly D_t, one ulp below and one above: a distance equal to D_t falls in the next bin."""
    mine = ev.RepeatabilityCounts(g["boundary_dist"].reshape(-1, 1))
    assert [int(c) for c in mine] == g["boundary_counts"].tolist() == [2, 6, 6, 6, 6, 6, 6, 4]


@pytest.mark.parametrize("step", STEPS)
def test_error_rts_match_reference(g, step):
    """GetErrorRTs (Visualization.py:163-172) of method 0 in every sequence at frame steps 1, 2 and 10, sliced [0:n:step]."""
    frames = seq_slices(g["n_frames"])
    tr = g["tr"]
    es, ts, sc = [], [], []
    for s, sl in enumerate(frames):
        _, _, e, t = ev.GetErrorRTs(g["gt_poses"][sl], g["est_poses"][0][sl].astype(np.float64), tr[s], step)
        assert e.dtype == np.float32 and t.dtype == np.float64
        es.append(e); ts.append(t)
        sc.append(np.full((t.shape[0], 1), 2 * np.abs(g["gt_poses"][sl].reshape(-1, 3, 4)[:, :, 3]).max()))
    n = [sum(len(range(0, sl.stop - sl.start, st)) - 1 for sl in frames) for st in STEPS]
    start = sum(n[:STEPS.index(step)])
    close(np.concatenate(es), g["err_eulers"][start:start + n[STEPS.index(step)]])
    close(np.concatenate(ts), g["err_ts"][start:start + n[STEPS.index(step)]], np.concatenate(sc))


def _rows(g, methods, step):
    frames = seq_slices(g["n_frames"])
    out = []
    reg = [tuple(m) for m in g["reg_methods"].tolist()]
    for k, d in methods:
        m = reg.index((k, d))
        seqs = []
        for s, sl in enumerate(frames):
            _, _, e, t = ev.GetErrorRTs(g["gt_poses"][sl], g["est_poses"][m][sl].astype(np.float64), g["tr"][s], step)
            pair = slice(sl.start - s, sl.stop - s - 1)
            mt = g["matchability"][m][:, pair].astype(np.int64)
            seqs.append((e, t) + ev.matchability_arrays(mt[0], mt[1], mt[2]))
        out.append(ev.RegistrationRow(seqs))
    return out


def test_registration_rows_match_evaluation_on_registration(g):
    """RegistrationRow == the 3 x 3 rows EvaluationOnRegistration.py wrote (success rate and inlier ratio as fractions)."""
    rows = _rows(g, [(k, d) for k in range(3) for d in range(3)], 1)
    ref = g["EvaluationResults"]
    for i, (row, ok) in enumerate(rows):
        assert row.dtype == np.float32 and row.shape == (7,)
        assert row[4] == ref[i, 4]                       # the success count is identical
        close(row, ref[i])
    assert 0.5 < ref[:, 4].min() and ref[:, 4].max() < 1.0   # the fixture has failures and successes in every method


@pytest.mark.parametrize("step", STEPS)
def test_registration_rows_match_eval_on_reg_keypts(g, step):
    """The rows of EvalOnReg_KeyPts.py (Descs = [2], six key point methods) at frame steps 1, 2 and 10; that script reports columns
    5 and 6 in percent."""
    rows = _rows(g, [(k, 2) for k in range(6)], step)
    ref = g["EvaluationResults_KeyPts_%d" % step]
    for k, (row, ok) in enumerate(rows):
        r = row.copy()
        r[4] = 100 * np.sum(ok) / ok.shape[0]
        r[5] = 100 * row[5]
        assert int(round(float(r[4]) * ok.shape[0] / 100)) == int(round(float(ref[k * 3 + 2, 4]) * ok.shape[0] / 100))
        close(r, ref[k * 3 + 2])


def test_matchability_file_round_trip(tmp_path):
    """AllProportions / AllTrialCounts [1, n] f64: the registration scripts read mat[...].T -> [n, 1]."""
    p = ev.save_matchability(str(tmp_path / "m.mat"), [10, 0, 7], [20, 5, 7], [3, 100, 1])
    prop, trials = ev.load_matchability(p)
    assert prop.shape == (1, 3) and trials.shape == (1, 3) and prop.dtype == np.float64 and trials.dtype == np.float64
    assert prop.T.shape == (3, 1) and prop.ravel().tolist() == [0.5, 0.0, 1.0] and trials.ravel().tolist() == [3.0, 100.0, 1.0]


def test_repeatability_file_round_trip(g, tmp_path):
    """{'counts': list of NumPy ints} -> what the reference's savemat call writes (shape and dtype recorded from its own files)."""
    counts = g["counts"][0, 0, 0, 0].tolist()
    p = ev.save_repeatability(str(tmp_path / ev.repeatability_name(1, "ae", "00")), [np.int64(c) for c in counts])
    assert os.path.basename(p) == "AccuracyOfKeyPts_1_0_00.mat"
    m = io.loadmat(p)["counts"]
    assert m.shape == tuple(g["counts_shape"]) and str(m.dtype) == str(g["counts_dtype"]) and m.ravel().tolist() == counts
    assert ev.repeatability_name(2, "usip", "07", inner=True) == "InnerAccuracyOfKeyPts_2_2_07.mat"


def _sets(ks):
    rng = np.random.default_rng(0)
    return [rng.uniform(-5, 5, (k, 3)) for k in ks]


def test_refuses_fit_sets_of_three_points_or_fewer():
    with pytest.raises(ValueError, match="3 or fewer"):
        ev.GetPairDistances(_sets([10, 3, 10]))
    with pytest.raises(ValueError, match="3 or fewer"):
        ev.ComputeDispersionOfKeypoints(_sets([10, 2]))


def test_refuses_non_finite_coordinates():
    s = _sets([10, 10])
    s[1][4, 2] = np.nan
    with pytest.raises(ValueError, match="NaN, infinity"):
        ev.GetPairDistances(s)
    s[1][4, 2] = np.inf
    with pytest.raises(ValueError, match="NaN, infinity"):
        ev.ComputeDispersionOfKeypoints(s)


def test_refuses_bad_thresholds_and_oversized_sets():
    with pytest.raises(ValueError, match="thresholds"):
        ev.device_distances(_sets([10, 10]), thresholds=[0.1, -1.0])
    with pytest.raises(ValueError, match="thresholds"):
        ev.device_distances(_sets([10, 10]), thresholds=[0.1] * 17)
    with pytest.raises(ValueError, match="at most"):
        ev.check_sets([np.zeros((65537, 3)), np.zeros((5, 3))], ev.pair_list(2))


def test_refuses_a_pose_count_that_does_not_match_the_frames(g, tree):
    d = tree / "00"
    gt = np.loadtxt(str(d / "gt.txt"))
    with pytest.raises(ValueError, match="poses for"):
        ev.GetAllKeyPts(str(d / "ae"), "ae", gt[:-1], ev.read_tr(str(d / "calib_.txt")))

