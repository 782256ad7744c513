"""CPU: the comparison protocol's registrar (csrc/adaptive.hip) through its host twin caelo_host_ransac_adaptive -- the same sample
rule, fit, inlier test and walk the kernel runs -- against the float64 NumPy restatement of the reference's MATLAB (tests/adaptive_ref.py):
the walk's integers and the inlier mask EQUAL, R and T within bars that only absorb rounding.  Also the sample rule at its edges, the
chaining rule with its carry-over on a failed first, middle and last pair, and run_sequence.py's flags and file names."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import adaptive_ref as ar  # noqa: E402
from caelo import _ffi, adaptive, framesteps as fs  # noqa: E402

CASES = list(ar.cases())
# Worst |host twin - restatement| over R, T, R_ransac, T_ransac per case, measured on the build machine (profiles/adaptive_errors.txt);
# the bar is 4 x that and never above 1e-7.  Both sides are float64: a wrong inlier, trial or tie moves these numbers by 1e-3 or more.
MEASURED_HOST = {
    "n2": 0.0, "n3": 7.327e-15, "n4": 3.553e-15, "n5": 2.190e-12, "n64": 4.663e-15, "n65": 7.105e-15, "n1000": 3.997e-15, "n1024": 4.441e-16,
    "trials_100": 1.243e-14, "trials_hundreds": 1.776e-14, "trials_thousands": 6.217e-15, "limit_n64": 0.0, "later_repeat": 2.665e-15,
    "past_the_stop": 2.220e-15, "duplicates": 3.553e-15, "same_frame": 0.0,
}


def test_the_case_list_names_what_the_issue_names():
    assert set(MEASURED_HOST) == set(CASES)
    assert [len(ar.cases()["n%d" % n][0]) for n in (2, 3, 4, 5, 64, 65, 1000, 1024)] == [2, 3, 4, 5, 64, 65, 1000, 1024]
    trials = {name: ar.reference(name)[0]["trials"] for name in ("trials_100", "trials_hundreds", "trials_thousands")}
    assert trials["trials_100"] == 100 and 200 <= trials["trials_hundreds"] < 1000 and 2000 <= trials["trials_thousands"] < 10000, trials
    x1, x2 = ar.cases()["duplicates"][:2]
    assert len(np.unique(x2, axis=0)) < len(x2) and np.array_equal(*ar.cases()["same_frame"][:2])


@pytest.mark.parametrize("name", CASES)
def test_restatement_is_far_from_every_decision_rounding_could_turn(name):
    ref, st = ar.reference(name)
    print("%s: trials %d, best %d, status %d, %d inliers; gaps: residual %.3g, singular values %.3g, N %.3g"
          % (name, ref["trials"], ref["best_trial"], ref["status"], len(ref["inliers"]), st["min_residual_gap"], st["min_sv_gap"], st["min_N_gap"]))
    assert st["min_residual_gap"] > 1e-6 and st["min_sv_gap"] > 1e-5 and st["min_N_gap"] > 1e-6
    want = ar.cases()[name][3]
    for key, value in (want or {}).items():
        got = len(ref["inliers"]) if key == "n_inliers" else ref[key]
        assert got == value, (name, key, got, value)


@pytest.mark.parametrize("name", CASES)
def test_host_twin_equals_the_restatement(name):
    x1, x2, draws, _ = ar.cases()[name]
    rec, mask = adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, draws)
    err = ar.compare(rec, mask, name)     # (trials, best_trial, status, n_inliers, n_pairs and the mask: ==)
    bar = min(4.0 * MEASURED_HOST[name], 1e-7)
    print("%s: worst |R, T, R_ransac, T_ransac - restatement| %.3e (bar %.3e)" % (name, err, bar))
    assert err <= bar


def test_limit_and_small_inputs_return_the_identity():
    x1, x2, draws, _ = ar.cases()["limit_n64"]
    rec, mask = adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, draws)
    eye = np.r_[np.eye(3).ravel(), np.zeros(3)]
    assert (rec["status"], rec["trials"], rec["n_inliers"], rec["best_trial"]) == (1, 10000, 0, -1) and not mask.any()
    assert np.array_equal(np.r_[rec["R"], rec["T"]], eye) and np.array_equal(np.r_[rec["R_ransac"], rec["T_ransac"]], eye)
    for n in (0, 1, 2):
        rec, mask = adaptive.host_ransac_adaptive(np.ones((n, 3)), np.ones((n, 3)), 1.0, draws)
        assert (rec["status"], rec["trials"], rec["n_inliers"], rec["n_pairs"]) == (2, 0, 0, n) and np.array_equal(np.r_[rec["R"], rec["T"]], eye)
    with pytest.raises(ValueError):
        adaptive.host_ransac_adaptive(np.ones((1025, 3)), np.ones((1025, 3)), 1.0, draws)
    with pytest.raises(ValueError):
        adaptive.host_ransac_adaptive(x1, x2, 1.0, draws[:100])


# ---- the sample rule -------------------------------------------------------------------------------------------------------------------
TOP = 1.0 - 2.0 ** -53


@pytest.mark.parametrize("n", [3, 4, 5, 1024])
def test_sample_rule_distinct_and_in_range(n):
    rs = np.random.RandomState(n)
    us = [np.array(u) for u in ((0, 0, 0), (TOP, TOP, TOP), (0, TOP, 0), (TOP, 0, TOP), (0, 0, TOP), (TOP, TOP, 0), (0.5, 0.5, 0.5))] + list(rs.random_sample((200, 3)))
    for u in us:
        idx = ar.sample_indices(u, n)
        assert len(set(idx)) == 3 and all(0 <= i < n for i in idx), (n, u, idx)
    assert ar.sample_indices((0, 0, 0), n) == (0, 1, 2) and ar.sample_indices((TOP, TOP, TOP), n) == (n - 1, n - 2, n - 3)
    if n <= 5:   # every ordered triple of distinct indices has its own cell of [0, 1)^3
        grid = [(a + 0.5) / 60 for a in range(60)]
        seen = {ar.sample_indices((a, b, c), n) for a in grid for b in grid for c in grid}
        assert len(seen) == n * (n - 1) * (n - 2)


@pytest.mark.parametrize("n", [4, 5, 1024])
def test_library_samples_by_the_same_rule(n):
    """A draw table that repeats ONE triple of draws: every trial fits the same three pairs, so R_ransac, T_ransac are the fit to the
    triple the rule names (any other triple of these clouds gives another motion) -- at u = 0, u = 1 - 2^-53 and in between."""
    x1, x2 = ar.make_pair(900 + n, n, 0.5, noise=0.3)
    rs = np.random.RandomState(50 + n)
    for u in [np.zeros(3), np.full(3, TOP), np.array([TOP, 0.0, TOP]), np.array([0.0, TOP, 0.0])] + list(rs.random_sample((6, 3))):
        rec, _ = adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, np.tile(u, (adaptive.DRAWS, 1)))
        ind = list(ar.sample_indices(u, n))
        want = ar.estimate_rt(x1.T[:, ind], x2.T[:, ind])
        got = np.c_[rec["R_ransac"].reshape(3, 3), rec["T_ransac"]]
        assert rec["status"] in (0, 1)
        if rec["status"] == 0:
            assert np.abs(got - want).max() < 1e-7, (n, u, ind)
            assert rec["best_trial"] == rec["trials"] - 1       # equal counts: the later trial wins, up to the last one walked


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def _chain_pairs(fail_at):
    good = [ar.make_pair(700 + k, 120, 0.6) for k in range(4)]
    bad = {"short": (np.ones((2, 3)), np.zeros((2, 3))), "limit": ar.make_pair(14, 64, 0.0)}
    pairs = list(good)
    for pos, kind in fail_at:
        pairs.insert(pos, bad[kind])
    return pairs


@pytest.mark.parametrize("fail_at", [[(0, "short")], [(2, "limit")], [(4, "short")], [(0, "limit"), (2, "short"), (6, "short")]],
                         ids=["first", "middle", "last", "first_middle_last"])
def test_chain_carries_the_previous_motion_over_a_failed_pair(fail_at):
    """The script applies the previous motion as a prior and composes the update with it; here the pairs are registered independently
    and a pair that is not solved repeats the motion before it (identity before the first solved pair): the same relative motions."""
    pairs, draws = _chain_pairs(fail_at), ar.base_draws(0)
    rel_ref, prop_ref, cnt_ref = ar.chain(pairs, ar.THRESHOLD, draws)
    recs = np.array([adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, draws)[0] for x1, x2 in pairs])
    rel, solved = adaptive.fit_rows(recs)
    got = adaptive.chain_relative(rel, solved)
    failed = sorted(pos for pos, _ in fail_at)
    assert np.flatnonzero(~solved).tolist() == failed
    assert np.array_equal(recs["trials"], cnt_ref) and np.array_equal(recs["n_inliers"] / recs["n_pairs"], prop_ref)
    assert np.abs(got - rel_ref).max() < 1e-9      # (the prior changes nothing but rounding: 1e-14 here)
    eye = np.r_[np.eye(3).ravel(), np.zeros(3)]
    for k in failed:
        assert np.array_equal(got[k], got[k - 1] if k else eye)


class _StubEngine:
    """Engine.register_pairs_adaptive's interface on CPU tensors: R[0], R[1] = the global frame numbers written into the two frames'
    rows; a pair whose frame a is a multiple of 7 fails (status 1)."""

    def __init__(self):
        self.calls = []

    def register_pairs_adaptive(self, rows, n_key, table, draws, threshold=1.0, desc=None):
        res = np.zeros(len(table), dtype=_ffi.ADAPTIVE_DTYPE)
        for q, (a, b) in enumerate(table):
            assert 0 <= a < rows.shape[0] and 0 <= b < rows.shape[0], "table index outside the resident window"
            fa, fb = float(rows[a, 0, 0]), float(rows[b, 0, 0])
            res["R"][q, 0], res["R"][q, 1], res["T"][q, 0] = fa, fb, threshold
            res["n_pairs"][q], res["n_inliers"][q], res["trials"][q] = int(n_key[a]), 50, 100 + int(fa)
            res["status"][q] = 1 if int(fa) % 7 == 0 else 0
        self.calls.append((int(rows.shape[0]), list(table), draws))
        return collections.namedtuple("Out", "results")(res)


@pytest.mark.parametrize("chunk", [8, 16])
def test_step_registrar_takes_the_registrar_as_a_parameter(chunk):
    """StepRegistrar(registrar=(draws, threshold)): every step, step 1 INCLUDED, goes through Engine.register_pairs_adaptive on the
    carried rows, every pair once and from the right frames; step_results chains with the carry-over."""
    import torch
    n, steps, draws = 40, [1, 5], "the draws"
    eng = _StubEngine()
    reg = fs.StepRegistrar(eng, steps, 0, True, 0, registrar=(draws, 0.75))
    assert reg.steps == [1, 5] and fs.StepRegistrar(eng, steps, 0, True, 0).steps == [5]
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        rows = torch.zeros((c1 - c0, 1024, 64))
        rows[:, 0, 0] = torch.arange(c0, c1, dtype=torch.float32)
        reg.keep(c0, collections.namedtuple("B", "k rows n_key")(c1 - c0, rows, torch.full((c1 - c0,), 100, dtype=torch.int32)))
    assert all(w <= 5 + chunk and d is draws for w, _, d in eng.calls)
    for s in steps:
        rel, ok, nin, npairs, its = reg.step_results(s)
        want = fs.step_pairs(n, s)
        assert len(rel) == len(want) and (npairs == 100).all() and (nin == 50).all() and rel.dtype == np.float64
        assert its.tolist() == [100 + a for a, _ in want] and ok.tolist() == [a % 7 != 0 for a, _ in want]
        last = (1.0, 0.0)                                           # the identity's R[0], R[1]
        for k, (a, b) in enumerate(want):
            last = (float(a), float(b)) if a % 7 else last          # a failed pair repeats the motion before it
            assert (rel[k, 0], rel[k, 1]) == last


# ---- run_sequence.py ---------------------------------------------------------------------------------------------------------------------
RS = os.path.join(REPO, "cae-lo_amd", "run_sequence.py")


def test_cli_flags_and_file_names(tmp_path):
    """--registrar comparison keeps every run's file names (--out and --matchability with '<s>_' in front for a step s) and refuses what
    it cannot do before any device work."""
    out, mat = str(tmp_path / "poses_" / "00.txt"), str(tmp_path / "m" / "Matchablity_00.mat")
    assert fs.step_path(out, 1) == out and fs.step_path(out, 5) == str(tmp_path / "poses_" / "5_00.txt")
    assert fs.step_path(mat, 5) == str(tmp_path / "m" / "5_Matchablity_00.mat")
    assert adaptive.REGISTRARS == ("match", "comparison")

    def refused(args, text):
        r = subprocess.run([sys.executable, RS, "--out", out] + args, capture_output=True, timeout=300)
        assert r.returncode == 2 and text in r.stderr.decode(), r.stderr.decode()[-2000:]
        assert not os.path.exists(out)

    refused(["--synthetic", "4", "--registrar", "comparison", "--inlier-threshold", "0"], "--inlier-threshold must be a positive")
    refused(["--synthetic", "4", "--registrar", "comparison", "--draw-seed", "-1"], "--draw-seed -1")
    refused(["--synthetic", "4", "--registrar", "comparison", "--save-artifacts"], "--registrar comparison runs on one GPU")
    refused(["--synthetic", "4", "--registrar", "comparison", "--gpus", "2"], "--registrar comparison runs on one GPU")
    refused(["--synthetic", "4", "--registrar", "ransac"], "invalid choice")
    # --calib-angle goes with --desc-dir under this registrar only
    refused(["--desc-dir", str(tmp_path), "--desc-dim", "8", "--features-from", str(tmp_path), "--calib-angle", "0.22"], "--calib-angle do not go with it")
    refused(["--desc-dir", str(tmp_path), "--desc-dim", "8", "--features-from", str(tmp_path), "--calib-angle", "0.22", "--registrar", "comparison"],
            "need at least frames 0 and 1")


def test_draw_table_is_numpys_stream():
    d = adaptive.draw_table(7)
    assert d.shape == (10001, 3) and np.array_equal(d, np.random.RandomState(7).random_sample((10001, 3)))
    with pytest.raises(ValueError):
        adaptive.draw_table(-1)


def test_abi_additions_without_a_device():
    import ctypes as C
    lib = _ffi.load()
    assert lib.caelo_abi_version() == 6
    header = open(os.path.join(REPO, "include", "caelo.h")).read()
    for name in ("caelo_ransac_adaptive", "caelo_host_ransac_adaptive", "caelo_register_pairs_adaptive", "caelo_register_pairs_adaptive_ws_bytes"):
        assert hasattr(lib, name) and name + "(" in header
    assert _ffi.ADAPTIVE_DTYPE.itemsize == 24 * 8 + 6 * 4
    assert lib.caelo_register_pairs_adaptive_ws_bytes(1, 60) == lib.caelo_register_pairs_adaptive_ws_bytes(100000, 60) >= 8 * lib.caelo_match_ws_bytes(1024)
    assert lib.caelo_register_pairs_adaptive_ws_bytes(5, 256) >= 8 * lib.caelo_match_ws_bytes_dim(1024, 256) and lib.caelo_register_pairs_adaptive_ws_bytes(-1, 60) == 0
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)

    def refused(text, ctx=None, rows=p, n_frames=2, pairs=p, n_pairs=1, draws=p):
        assert lib.caelo_register_pairs_adaptive(ctx, rows, n_frames, p, pairs, n_pairs, draws, 1.0, p, p, p, p, None, None, 64, 60) < 0
        assert text in lib.caelo_last_error().decode(), lib.caelo_last_error()

    refused("null pair table", pairs=None)
    refused("n_frames", n_frames=0)
    refused("n_pairs", n_pairs=-1)
    refused("null argument")                 # no context
    assert lib.caelo_host_ransac_adaptive(p, p, 1025, p, 1.0, p, p) < 0 and "n must lie in [0, 1024]" in lib.caelo_last_error().decode()
    assert lib.caelo_ransac_adaptive(None, p, p, 4, p, 1.0, p, p, None, None) < 0 and "null argument" in lib.caelo_last_error().decode()
