"""CPU: the comparison protocol's registrar at the edges of its own construction, through the host twin caelo_host_ransac_adaptive
(tests/test_adaptive_edges_gpu.py runs the same inputs through k_adaptive and against this twin).  tests/adaptive_ref.py builds the
inputs: walks planted to stop at 127 .. 129, 256, 257, 9984, 9985, at the limit and one past it, with the best trial in the chunk
slots 0, 63, 64, 127 and the first slot of the next chunk; residuals known to the bit at, one step below and one step above the
threshold; triples that leave the rotation open or hold a NaN; the sample rule at u = 0 and u = 1 - 2^-53.  Every expectation is
asserted on the float64 restatement (or derived by hand) before the library is looked at."""
import itertools
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cae-lo_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import adaptive_ref as ar  # noqa: E402
from caelo import adaptive  # noqa: E402

PLANTED = list(ar.PLANTED)
BAR = 1e-7      # the project's cap.  Both sides are float64: a wrong trial or inlier moves R, T by 1e-3 or more
EYE = np.r_[np.eye(3).ravel(), np.zeros(3)]


def rt(rec, which=""):
    return np.r_[rec["R" + which], rec["T" + which]]


def facts(rec):
    return dict(trials=int(rec["trials"]), best_trial=int(rec["best_trial"]), status=int(rec["status"]), n_inliers=int(rec["n_inliers"]))


# ---- 1. planted walks ----------------------------------------------------------------------------------------------------------------
def test_the_enumeration_finds_the_windows_the_cases_need():
    for name in PLANTED:
        where = ar.PLANTED[name][0]
        n, c, N = ar.planted_nc(name)
        print("%-30s n %4d  c %3d  N %.2f" % (name, n, c, N))
        if where[0] == "window":
            assert where[1] - 1 < N < where[1] and where[2] <= n <= where[3] and N == ar.trials_needed(c, n)
            if where[1] < 1000:
                assert 0.2 < N - (where[1] - 1) < 0.8      # (near the limit the enumeration has one or two pairs to offer)
        else:
            assert N < 100
    assert ar.planted_nc("stop_128_n_small")[0] % 64 and ar.planted_nc("stop_128_n_large")[0] >= 1000
    assert ar.find_nc(10000) is None                       # no (n, c) up to 1024 has its N in (9999, 10000)


@pytest.mark.parametrize("name", PLANTED)
def test_planted_walk_does_on_the_restatement_what_the_registry_says(name):
    x1, x2, draws, _, want, want_mask = ar.edge_cases()[name]
    n, c, _ = ar.planted_nc(name)
    good = set(ar.PLANTED[name][1])
    inl = ar.planted_inputs(name)[3].astype(bool)
    assert len(x1) == n and inl.sum() == c
    for t in sorted(good | {0, 1, 127, 128, 129, 9983, 9984, 9999, 10000}):
        assert bool(inl[list(ar.sample_indices(draws[t], n))].all()) == (t in good), t
    ref, st = ar.edge_reference(name)
    print("%s: trials %d, best %d, status %d, %d inliers; gaps: residual %.3g, singular values %.3g, N %.3g"
          % (name, ref["trials"], ref["best_trial"], ref["status"], len(ref["inliers"]), st["min_residual_gap"], st["min_sv_gap"], st["min_N_gap"]))
    assert st["min_residual_gap"] > 1e-6 and st["min_sv_gap"] > 1e-5 and st["min_N_gap"] > 1e-6
    assert dict(trials=ref["trials"], best_trial=ref["best_trial"], status=ref["status"], n_inliers=len(ref["inliers"])) == want
    mask = np.zeros(n, np.uint8)
    mask[ref["inliers"]] = 1
    assert np.array_equal(mask, want_mask)                 # status 0: the planted inlier set exactly


@pytest.mark.parametrize("name", PLANTED)
def test_host_twin_walks_the_planted_case(name):
    x1, x2, draws, t, want, want_mask = ar.edge_cases()[name]
    rec, mask = adaptive.host_ransac_adaptive(x1, x2, t, draws)
    assert facts(rec) == want and np.array_equal(mask, want_mask)
    err = ar.compare_edge(rec, mask, name)
    print("adaptive_errors %-30s %.3e (bar %.3e)" % (name, err, BAR))
    assert err <= BAR
    if want["status"] == 1:
        assert np.array_equal(rt(rec), EYE) and np.array_equal(rt(rec, "_ransac"), EYE)
    else:                                                  # the best trial's model is the fit to THAT trial's triple
        ind = list(ar.sample_indices(draws[want["best_trial"]], len(x1)))
        assert ar.rt_error(rec, ar.edge_reference(name)[0]["Rt"], ar.estimate_rt(x1.T[:, ind], x2.T[:, ind])) <= BAR


# ---- 2. the threshold, exactly -------------------------------------------------------------------------------------------------------
def check_threshold_band(rec, mask, t):
    """The expectation is exact: the hand-computed mask, the identity as the best trial's model, the last trial walked the best."""
    x1, x2, _, want = ar.threshold_band(t)
    n, count = len(x1), int(want.sum())
    N = ar.trials_needed(count, n)
    assert 100.5 < N < 256 and abs(N - np.round(N)) > 0.1
    assert np.array_equal(mask, want), np.flatnonzero(mask != want)
    trials = int(np.ceil(N))
    assert facts(rec) == dict(trials=trials, best_trial=trials - 1, status=0, n_inliers=count)
    assert np.array_equal(rt(rec, "_ransac"), EYE)
    sel = np.flatnonzero(want)
    assert ar.rt_error(rec, ar.estimate_rt(x1.T[:, sel], x2.T[:, sel]), ar.IDENTITY) <= BAR


@pytest.mark.parametrize("t", [1.0, 5.0])
def test_threshold_band_inputs_say_what_they_should(t):
    x1, x2, draws, want = ar.threshold_band(t)
    e = x1 - x2
    m = 12
    assert np.array_equal(x1[:m], x2[:m]) and want[:m].all()
    probes = {tuple(v): bool(w) for v, w in zip(e[m:], want[m:])}
    lo, hi = np.nextafter(t, 0.0), np.nextafter(t, np.inf)
    for axis in range(3):
        for v, inside in ((t, False), (lo, True), (hi, False), (-t, False), (-lo, True), (-hi, False)):
            assert probes[tuple(np.eye(3)[axis] * v)] == inside
    assert lo * lo > t * t * (1.0 - 2.0 ** -50)            # inside the band: the square root decides
    if t == 5.0:
        assert probes[(3.0, 4.0, 0.0)] is False
        # one ulp below 25, the correctly rounded root is 5.0: out, although the true distance is below t and s < t * t
        below = np.nextafter(4.0, 0.0)
        assert 9.0 + below * below < 25.0 and np.sqrt(9.0 + below * below) == 5.0 and probes[(3.0, below, 0.0)] is False
    assert 0 < want[m:].sum() < len(probes)


@pytest.mark.parametrize("t", [1.0, 5.0])
def test_host_twin_at_the_threshold(t):
    x1, x2, draws, _ = ar.threshold_band(t)
    check_threshold_band(*adaptive.host_ransac_adaptive(x1, x2, t, draws), t)


THRESHOLD_VALUES = [("zero", 0.0), ("negative", -1.0), ("nan", float("nan")), ("inf", float("inf")), ("1e200", 1e200), ("1e-200", 1e-200)]


def threshold_value_input(name):
    return ar.cases()["same_frame" if name == "1e-200" else "n65"][:3]


def check_threshold_value(rec, mask, name):
    x1, x2, draws = threshold_value_input(name)
    n = len(x1)
    if name in ("zero", "negative", "nan"):                # no pair is ever an inlier
        assert facts(rec) == dict(trials=10000, best_trial=-1, status=1, n_inliers=0) and not mask.any()
        assert np.array_equal(rt(rec), EYE) and np.array_equal(rt(rec, "_ransac"), EYE)
        return
    assert facts(rec) == dict(trials=100, best_trial=99, status=0, n_inliers=n) and mask.all()
    if name == "1e-200":                                    # s = 0 exactly: t * t underflows to 0, the square root decides
        assert np.array_equal(rt(rec), EYE) and np.array_equal(rt(rec, "_ransac"), EYE)
    else:
        ind = list(ar.sample_indices(draws[99], n))
        assert ar.rt_error(rec, ar.estimate_rt(x1.T, x2.T), ar.estimate_rt(x1.T[:, ind], x2.T[:, ind])) <= BAR


@pytest.mark.parametrize("name,t", THRESHOLD_VALUES, ids=[v[0] for v in THRESHOLD_VALUES])
def test_host_twin_threshold_values(name, t):
    x1, x2, draws = threshold_value_input(name)
    check_threshold_value(*adaptive.host_ransac_adaptive(x1, x2, t, draws), name)


# ---- 3. degenerate and non-finite triples --------------------------------------------------------------------------------------------
def check_degenerate(rec, mask, name):
    x1, x2, _ = ar.degenerate_inputs()[name]
    assert facts(rec)["status"] == 0 and facts(rec)["trials"] == 100 and facts(rec)["best_trial"] == 99
    if name == "one_pair_thrice":                           # the matrix is exactly zero: the identity, T = x - y
        want = np.r_[np.eye(3).ravel(), x1[0] - x2[0]]
        assert np.array_equal(rt(rec, "_ransac"), want) and np.array_equal(rt(rec), want)
        assert facts(rec)["n_inliers"] == 3 and mask.tolist() == [1, 1, 1, 0, 0]
        return
    R, T = rec["R_ransac"].reshape(3, 3), rec["T_ransac"]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
    if name == "shared_y":                                  # the fit leaves no more than the true motion does: the triple is in
        assert facts(rec)["n_inliers"] >= 3 and mask[:3].all()
    if name == "collinear_rigid":                           # whichever rotation about the line: the model maps the triple onto itself
        assert np.abs((R @ x2[:3].T).T + T - x1[:3]).max() <= 1e-9
        assert facts(rec)["n_inliers"] >= 3 and mask[:3].all()


@pytest.mark.parametrize("name", list(ar.degenerate_inputs()))
def test_host_twin_on_degenerate_triples(name):
    x1, x2, draws = ar.degenerate_inputs()[name]
    assert ar.sample_indices(draws[0], len(x1)) == (0, 1, 2) and 4 <= len(x1) <= 8
    check_degenerate(*adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, draws), name)


def check_nonfinite(rec, mask, name):
    x1, x2, _, bad = ar.nonfinite_inputs()[name]
    want, want_mask = ar.nonfinite_expected(name)
    assert mask[bad] == 0
    assert facts(rec) == want and np.array_equal(mask, want_mask)
    assert np.isfinite(rt(rec)).all() and np.isfinite(rt(rec, "_ransac")).all()
    keep = np.flatnonzero(want_mask)
    ind = list(ar.sample_indices(ar.nonfinite_inputs()[name][2][want["best_trial"]], len(x1)))
    assert ar.rt_error(rec, ar.estimate_rt(x1.T[:, keep], x2.T[:, keep]), ar.estimate_rt(x1.T[:, ind], x2.T[:, ind])) <= BAR


@pytest.mark.parametrize("name", list(ar.nonfinite_inputs()))
def test_host_twin_never_counts_a_pair_that_is_not_finite(name):
    x1, x2, draws, bad = ar.nonfinite_inputs()[name]
    n = len(x1)
    sampled = [bad in ar.sample_indices(draws[t], n) for t in range(100)]
    assert any(sampled) and not all(sampled)               # the walk meets both kinds of trial
    check_nonfinite(*adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, draws), name)


# ---- 4. the sample rule --------------------------------------------------------------------------------------------------------------
def check_sample_rule(rec, n, u):
    """Every trial fits the same three pairs: R_ransac, T_ransac are the fit to the triple the rule names (any other triple of the
    cloud gives another motion), and among equal counts the last trial walked is the best."""
    x1, x2, _ = ar.sample_rule_inputs(n)
    ind = list(ar.sample_indices(u, n))
    want = ar.estimate_rt(x1.T[:, ind], x2.T[:, ind])
    count = len(ar._inliers(want, x1.T, x2.T, ar.THRESHOLD, None))
    assert ar.trials_needed(count, n) < 9000               # (the restatement's own count: the walk ends below the limit)
    assert rec["status"] == 0 and rec["best_trial"] == rec["trials"] - 1
    assert np.abs(np.c_[rec["R_ransac"].reshape(3, 3), rec["T_ransac"]] - want).max() < BAR, (n, u, ind)


@pytest.mark.parametrize("n", [4, 5, 1024])
def test_host_twin_samples_the_edge_draws_of_the_device_test(n):
    x1, x2, us = ar.sample_rule_inputs(n)
    assert ar.sample_indices(us[0], n) == (0, 1, 2) and ar.sample_indices(us[1], n) == (n - 1, n - 2, n - 3)
    assert all(np.floor(ar.TOP * m) == m - 1 for m in (n, n - 1, n - 2))    # the largest draw names the last index, unclamped
    fits = {}                                              # one per SET of three pairs: another set gives another motion
    for ind in itertools.combinations(range(n), 3) if n <= 5 else {tuple(sorted(ar.sample_indices(u, n))) for u in us}:
        fits[ind] = ar.estimate_rt(x1.T[:, list(ind)], x2.T[:, list(ind)])
    assert min(np.abs(fits[a] - fits[b]).max() for a in fits for b in fits if a < b) > 1e-3
    for u in us:
        rec, _ = adaptive.host_ransac_adaptive(x1, x2, ar.THRESHOLD, ar.repeat_draw(u))
        check_sample_rule(rec, n, u)
