"""GPU: the comparison protocol's registrar (csrc/adaptive.hip, k_adaptive) against the float64 NumPy restatement of the reference's
MATLAB (tests/adaptive_ref.py, the cases of tests/test_adaptive_host.py): the walk's integers and the inlier mask EQUAL, R and T within
bars that only absorb rounding; Engine.register_pairs_adaptive on a mixed table against its single calls, bit for bit; and
run_sequence.py --desc-dir --registrar comparison against the restatement's chain."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import adaptive_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = list(ar.cases())
# Worst |device - restatement| over R, T, R_ransac, T_ransac per case, measured on an MI355X (profiles/adaptive_errors.txt); the bar is
# 4 x that and never above 1e-7.  Both sides are float64: a wrong inlier, trial or tie moves these numbers by 1e-3 or more.
MEASURED_GPU = {
    "n2": 0.000e+00, "n3": 7.327e-15, "n4": 3.553e-15, "n5": 2.190e-12,
    "n64": 4.663e-15, "n65": 7.105e-15, "n1000": 3.997e-15, "n1024": 1.998e-15,
    "trials_100": 1.243e-14, "trials_hundreds": 1.776e-14, "trials_thousands": 6.217e-15, "limit_n64": 0.000e+00,
    "later_repeat": 3.331e-15, "past_the_stop": 3.553e-15, "duplicates": 3.997e-15, "same_frame": 0.000e+00,
}


@pytest.fixture(scope="module")
def draws_dev(engine):
    """The draw tables of the cases on the device, one upload per distinct table."""
    cache = {}

    def get(d):
        if id(d) not in cache:
            cache[id(d)] = torch.from_numpy(d).to(engine.device)
        return cache[id(d)]
    return get


@pytest.mark.parametrize("name", CASES)
def test_engine_equals_the_restatement(engine, draws_dev, name):
    x1, x2, draws, _ = ar.cases()[name]
    rec, mask = engine.ransac_adaptive(x1, x2, draws_dev(draws), ar.THRESHOLD)
    err = ar.compare(rec, mask, name)     # (trials, best_trial, status, n_inliers, n_pairs and the mask: ==)
    bar = min(4.0 * MEASURED_GPU[name], 1e-7)
    print("adaptive_errors %-18s %.3e (bar %.3e)" % (name, err, bar))
    assert err <= bar


def test_device_trial_fits_are_the_host_twins(engine, draws_dev):
    """The best trial's model is the same operations on both sides: the device's R_ransac, T_ransac against the host twin's."""
    from caelo import adaptive
    for name in ("n5", "n65", "trials_hundreds", "duplicates"):
        x1, x2, draws, _ = ar.cases()[name]
        rec, mask = engine.ransac_adaptive(x1, x2, draws_dev(draws), ar.THRESHOLD)
        host, hmask = adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, draws)
        assert np.array_equal(mask, hmask) and all(rec[f] == host[f] for f in ("trials", "best_trial", "status", "n_inliers"))
        assert np.abs(np.r_[rec["R_ransac"], rec["T_ransac"]] - np.r_[host["R_ransac"], host["T_ransac"]]).max() <= 1e-12


def test_api_under_the_references_name(engine):
    from caelo import adaptive, api
    x1, x2, _, _ = ar.cases()["n65"]
    Rt, inliers, trials = api.RansacFitRt(x1.T, x2.T, ar.THRESHOLD, seed=0)     # the script's [3, n] layout; seed 0 = the cases' table
    ref, _ = ar.reference("n65")
    assert np.array_equal(adaptive.draw_table(0), ar.base_draws(0))
    assert Rt.shape == (3, 4) and np.array_equal(inliers, ref["inliers"]) and trials == ref["trials"] and np.abs(Rt - ref["Rt"]).max() < 1e-7
    Rt, inliers, trials = api.RansacFitRt(np.ones((3, 2)), np.ones((3, 2)), 1.0)
    assert Rt.shape == (0, 4) and len(inliers) == 0 and trials == 0


# ---- a table ----------------------------------------------------------------------------------------------------------------------------
F_TABLE = 8
TABLE = [(0, 1), (6, 0), (1, 2), (7, 3), (2, 2), (3, 0), (0, 5), (4, 1), (5, 4), (1, 6), (2, 3)]    # 11 pairs, not in slice order


def _table_frames():
    """Eight frames as rows (host): 0 .. 5 are 150 to 200 points of one cloud, moved, jittered and shuffled, with the cloud's
    descriptors (columns 0:60) slightly perturbed -- the match finds the partner; frame 6 holds 64 unrelated points (a pair that starts
    from it runs into the trial limit), frame 7 three points (the direct fit)."""
    rs = np.random.RandomState(77)
    base = rs.uniform(-40, 40, (220, 3)) * np.array([1.0, 1.0, 0.1])
    feat = rs.uniform(-1, 1, (220, 60))
    rows, nk = np.zeros((F_TABLE, 1024, 64), np.float32), np.zeros(F_TABLE, np.int32)
    for f in range(F_TABLE):
        if f <= 5:
            k = 150 + 10 * f
            pick = rs.permutation(220)[:k]
            R, T = ar.random_rigid(rs)
            pts, d = (R @ base[pick].T).T + T + 0.05 * rs.standard_normal((k, 3)), feat[pick] + 0.01 * rs.standard_normal((k, 60))
        else:
            k = 64 if f == 6 else 3
            pts, d = rs.uniform(-40, 40, (k, 3)) * np.array([1.0, 1.0, 0.1]), rs.uniform(-1, 1, (k, 60))
        rows[f, :k, 0:60], rows[f, :k, 60:63], rows[f, :k, 63], nk[f] = d, pts, 1.0, k
    return rows, nk


@pytest.fixture(scope="module")
def frames(engine):
    rows, nk = _table_frames()
    return dict(rows=torch.from_numpy(rows).to(engine.device), n_key=torch.from_numpy(nk).to(engine.device), rows_h=rows, nk=nk)


def _argmin_f64(desc_a, desc_b):
    """For each row of a the first nearest row of b in float64."""
    a, b = desc_a.astype(np.float64), desc_b.astype(np.float64)
    return np.array([int(np.argmin(np.sqrt(((b - r) ** 2).sum(axis=1)))) for r in a], dtype=np.int64)


def test_table_equals_its_single_calls(engine, frames, draws_dev):
    from caelo import _ffi
    draws = ar.base_draws(0)
    out = engine.register_pairs_adaptive(frames["rows"], frames["n_key"], TABLE, draws_dev(draws), ar.THRESHOLD)
    idx = out.pair_idx.cpu().numpy()
    assert out.results.dtype == _ffi.ADAPTIVE_DTYPE and len(out.results) == len(TABLE) > 8 and out.masks.shape == (len(TABLE), 1024)
    rows_h, nk = frames["rows_h"], frames["nk"]
    for q, (a, b) in enumerate(TABLE):
        n = int(nk[a])
        # the match: for each point of frame a the float64 argmin over frame b = caelo_match with the two frames exchanged
        want_idx = _argmin_f64(rows_h[a, :n, 0:60], rows_h[b, :nk[b], 0:60])
        assert np.array_equal(idx[q, :n], want_idx), (q, a, b)
        got = engine.match(frames["rows"][b, :, 0:60], frames["rows"][a, :, 0:60], frames["n_key"][b:b + 1], frames["n_key"][a:a + 1]).cpu().numpy()
        assert np.array_equal(idx[q, :n], got[:n])
        if a == b:
            assert np.array_equal(idx[q, :n], np.arange(n))
        # the pair's single call, bit for bit, in the table's order
        x1, x2 = rows_h[a, :n, 60:63].astype(np.float64), rows_h[b, idx[q, :n], 60:63].astype(np.float64)
        rec, mask = engine.ransac_adaptive(x1, x2, draws_dev(draws), ar.THRESHOLD)
        assert rec.tobytes() == out.results[q].tobytes(), (q, a, b)
        assert np.array_equal(out.masks[q, :n], mask) and not out.masks[q, n:].any()
        assert out.results["n_pairs"][q] == n and out.status[q] == rec["status"] and out.evals[q] == rec["trials"]
    st = {ab: (int(out.results["status"][q]), int(out.results["trials"][q]), int(out.results["n_inliers"][q])) for q, ab in enumerate(TABLE)}
    assert st[(0, 1)][:2] == (0, 100) and st[(0, 1)][2] > 100            # a 100-trial pair
    assert st[(6, 0)] == (1, 10000, 0)                                    # a limit pair
    assert st[(7, 3)] == (0, 0, 3)                                        # the direct fit on three pairs
    assert st[(2, 2)] == (0, 100, int(nk[2]))                             # the pair (f, f): the identity
    r = out.results[TABLE.index((2, 2))]
    assert np.array_equal(np.r_[r["R"], r["T"]], np.r_[np.eye(3).ravel(), np.zeros(3)])


def test_table_refusals(engine, frames, draws_dev):
    from caelo import _ffi
    d = draws_dev(ar.base_draws(0))
    with pytest.raises(_ffi.CaeloError, match="outside"):
        engine.register_pairs_adaptive(frames["rows"], frames["n_key"], [(0, F_TABLE)], d)
    empty = engine.register_pairs_adaptive(frames["rows"], frames["n_key"], np.zeros((0, 2), np.int64), d)
    assert len(empty.results) == 0


# ---- run_sequence.py --desc-dir --registrar comparison ---------------------------------------------------------------------------------
RS = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")
N_SEQ, DIM, ANGLE = 12, 32, 0.22


def _sequence_clouds():
    """-> [(key points [k, 3], descriptors [k, DIM])] of the 12 frames; frame 6 is unrelated to the others."""
    rs = np.random.RandomState(5)
    base = rs.uniform(-40, 40, (200, 3)) * np.array([1.0, 1.0, 0.1])
    feat = rs.uniform(-1, 1, (200, DIM))
    out = []
    for f in range(N_SEQ):
        if f == 6:
            pts, d = rs.uniform(-40, 40, (48, 3)) * np.array([1.0, 1.0, 0.1]), rs.uniform(-1, 1, (48, DIM))
        else:
            pick = rs.permutation(200)[:120 + 5 * f]
            R, T = ar.random_rigid(rs, angle=0.05, shift=1.0)
            pts, d = (R @ base[pick].T).T + T + 0.05 * rs.standard_normal((len(pick), 3)), feat[pick] + 0.01 * rs.standard_normal((len(pick), DIM))
        out.append((pts, d))
    return out


def test_cli_desc_dir_equals_the_restatements_chain(engine, tmp_path):
    """12 frames of 3DFeatNet-style key point files and 32-d descriptor files, frame 6 unrelated to its neighbours (the pairs (5, 6)
    and (6, 7) fail; step 5 never meets it): --registrar comparison --frame-steps 1,5 --calib-angle writes the poses the existing
    chain code makes of the restatement's relative motions (prior applied as the script applies it, key points corrected by the
    device CorrectPC) and the restatement's proportions and trial counts."""
    from caelo import adaptive, evaluate as ev, framesteps as fs, keysources, stageio
    kps, descs = [], []
    for f, (pts, d) in enumerate(_sequence_clouds()):
        keysources.write_3dfeatnet(keysources.keypts_path(str(tmp_path / "kp"), f), pts)
        keysources.write_descriptors(keysources.desc_path(str(tmp_path / "desc"), f), d)
        kps.append(keysources.load_keypts("3dfeatnet", str(tmp_path / "kp"), f))
        descs.append(keysources.read_descriptors(keysources.desc_path(str(tmp_path / "desc"), f), DIM))
    out, mat = tmp_path / "poses_" / "00.txt", tmp_path / "m" / "00.mat"
    r = subprocess.run([sys.executable, RS, "--desc-dir", str(tmp_path / "desc"), "--desc-dim", str(DIM), "--keypts-source", "3dfeatnet",
                        "--keypts-dir", str(tmp_path / "kp"), "--registrar", "comparison", "--frame-steps", "1,5", "--calib-angle", str(ANGLE),
                        "--chunk", "5", "--matchability", str(mat), "--out", str(out)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    moved = [engine.correct_pc(torch.from_numpy(k).to(engine.device), ANGLE).cpu().numpy().astype(np.float64) for k in kps]
    draws = adaptive.draw_table(0)
    for s in (1, 5):
        pairs = []
        for a, b in fs.step_pairs(N_SEQ, s):
            idx = _argmin_f64(descs[a], descs[b])
            pairs.append((moved[a], moved[b][idx]))
        rel, prop, cnt = ar.chain(pairs, 1.0, draws)
        if s == 1:
            assert cnt[5] == cnt[6] == 10000 and prop[5] == prop[6] == 0 and (np.delete(cnt, [5, 6]) < 10000).all()
            assert np.array_equal(rel[5], rel[4]) and np.array_equal(rel[6], rel[4])
        want = fs.expand_rows(stageio.chain_poses(rel, None), N_SEQ, s)
        got = np.loadtxt(fs.step_path(str(out), s)).reshape(-1, 12)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-5, (s, np.abs(got - want).max())   # (float32 poses of motions equal to 1e-12)
        p_got, c_got = ev.load_matchability(fs.step_path(str(mat), s))
        assert np.array_equal(np.ravel(p_got), prop) and np.array_equal(np.ravel(c_got), cnt.astype(np.float64))


def test_cli_pipeline_path_registers_every_step_from_the_resident_rows(engine, scans, tmp_path):
    """run_sequence.py --synthetic 7 --registrar comparison --frame-steps 1,5: step 1 and step 5 are both
    Engine.register_pairs_adaptive on the pipeline's rows, chained by the script's rule -- the files of a direct call here."""
    from caelo import adaptive, evaluate as ev, framesteps as fs, stageio
    from caelo.engine import ransac_draws
    n = 7
    out, mat = tmp_path / "poses_" / "00.txt", tmp_path / "m" / "00.mat"
    r = subprocess.run([sys.executable, RS, "--synthetic", str(n), "--trajectory", "line", "--registrar", "comparison", "--inlier-threshold", "0.8",
                        "--draw-seed", "3", "--frame-steps", "1,5", "--chunk", "4", "--matchability", str(mat), "--out", str(out)],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    pcs = [torch.from_numpy(scans(f)).to(engine.device) for f in range(n)]
    batch = engine.pipeline(8).run(pcs, [torch.from_numpy(ransac_draws(f)).to(engine.device) for f in range(n)], certify=False)
    rows, n_key = batch.rows[:n].contiguous(), batch.n_key[:n].contiguous()
    for s in (1, 5):
        res = engine.register_pairs_adaptive(rows, n_key, fs.step_pairs(n, s), adaptive.draw_table(3), 0.8)
        rel, ok, nin, npairs, its = fs.pack_results([(np.arange(len(res.results)), res.results)], s)
        assert ok.all() and (its >= 100).all()
        want = tmp_path / ("want_%d.txt" % s)
        stageio.write_poses(str(want), fs.expand_rows(stageio.chain_poses(rel, None), n, s))
        assert open(fs.step_path(str(out), s), "rb").read() == open(str(want), "rb").read()
        p_got, c_got = ev.load_matchability(fs.step_path(str(mat), s))
        assert np.array_equal(np.ravel(p_got), nin / npairs) and np.array_equal(np.ravel(c_got), its.astype(np.float64))
