"""GPU: k_adaptive (csrc/adaptive.hip) at the edges of its own construction -- the 128 trials it scores ahead of the walk, the two count
registers per lane, the walk's state crossing chunks through LDS, the short last chunk, the square root inside the threshold's band,
triples that leave the rotation open or hold a NaN, the sample rule's edge draws.  The inputs and their expectations are those of
tests/test_adaptive_edges_host.py (asserted there on the float64 restatement before the library is looked at); every input runs here
against the restatement or the hand-derived expectation AND against the host twin: the integers and the mask EQUAL, R_ransac and
T_ransac within 1e-12.  One launch is one workgroup."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests"))
import adaptive_ref as ar  # noqa: E402
import test_adaptive_edges_host as eh  # noqa: E402
import test_adaptive_gpu as tg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(engine):
    """(x1, x2, draws, t) -> (device record, device mask) after the device result was held against the host twin's."""
    from caelo import adaptive
    cache = {}

    def up(d):
        if id(d) not in cache:
            cache[id(d)] = (d, torch.from_numpy(d).to(engine.device))     # (the host array is kept: its id stays its own)
        return cache[id(d)][1]

    def go(x1, x2, draws, t):
        rec, mask = engine.ransac_adaptive(x1, x2, up(draws), t)
        host, hmask = adaptive.host_ransac_adaptive(x1, x2, t, draws)
        ar.same_walk(rec, mask, host, hmask)
        return rec, mask
    go.up = up
    return go


# ---- 1. planted walks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eh.PLANTED)
def test_engine_walks_the_planted_case(run, name):
    x1, x2, draws, t, want, want_mask = ar.edge_cases()[name]
    rec, mask = run(x1, x2, draws, t)
    assert eh.facts(rec) == want and np.array_equal(mask, want_mask)
    err = ar.compare_edge(rec, mask, name)
    print("adaptive_errors %-30s %.3e (bar %.3e)" % (name, err, eh.BAR))
    assert err <= eh.BAR
    if want["status"] == 1:
        assert np.array_equal(eh.rt(rec), eh.EYE) and np.array_equal(eh.rt(rec, "_ransac"), eh.EYE)
    else:                                                  # the best trial's model is the fit to THAT trial's triple
        ind = list(ar.sample_indices(draws[want["best_trial"]], len(x1)))
        assert ar.rt_error(rec, ar.edge_reference(name)[0]["Rt"], ar.estimate_rt(x1.T[:, ind], x2.T[:, ind])) <= eh.BAR


# ---- 2. the threshold, exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1.0, 5.0])
def test_engine_at_the_threshold(run, t):
    x1, x2, draws, _ = ar.threshold_band(t)
    eh.check_threshold_band(*run(x1, x2, draws, t), t)


@pytest.mark.parametrize("name,t", eh.THRESHOLD_VALUES, ids=[v[0] for v in eh.THRESHOLD_VALUES])
def test_engine_threshold_values(run, name, t):
    x1, x2, draws = eh.threshold_value_input(name)
    eh.check_threshold_value(*run(x1, x2, draws, t), name)


# ---- 3. degenerate and non-finite triples --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ar.degenerate_inputs()))
def test_engine_on_degenerate_triples(run, name):
    x1, x2, draws = ar.degenerate_inputs()[name]
    eh.check_degenerate(*run(x1, x2, draws, ar.THRESHOLD), name)


@pytest.mark.parametrize("name", list(ar.nonfinite_inputs()))
def test_engine_never_counts_a_pair_that_is_not_finite(run, name):
    x1, x2, draws, _ = ar.nonfinite_inputs()[name]
    eh.check_nonfinite(*run(x1, x2, draws, ar.THRESHOLD), name)


# ---- 4. the sample rule on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 1024])
def test_engine_samples_by_the_same_rule(run, n):
    x1, x2, us = ar.sample_rule_inputs(n)
    for u in us:
        rec, _ = run(x1, x2, ar.repeat_draw(u), ar.THRESHOLD)
        eh.check_sample_rule(rec, n, u)


# ---- 5. nothing outside the outputs, same bytes twice ----------------------------------------------------------------------------------
REC = 216      # bytes of a result record
GUARD = 64


@pytest.mark.parametrize("n", [0, 3, 5, 67, 1024])
def test_nothing_outside_the_record_and_the_mask(engine, run, n):
    """The entry point itself, outputs in the middle of buffers filled with 0xA5: the middle record of three and mask[0:n] are written,
    nothing before or behind them."""
    x1, x2 = ar.make_pair(300 + n, max(n, 1), 1.0 if n <= 5 else 0.6)
    x1, x2, draws = x1[:n], x2[:n], ar.base_draws(0)
    dev = engine.device
    res = torch.full((3 * REC,), 0xA5, dtype=torch.uint8, device=dev)
    mask = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    a, b = torch.from_numpy(np.ascontiguousarray(x1)).to(dev), torch.from_numpy(np.ascontiguousarray(x2)).to(dev)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    assert engine.lib.caelo_ransac_adaptive(engine.ctx, ptr(a) if n else None, ptr(b) if n else None, n, ptr(run.up(draws)), ar.THRESHOLD,
                                            ptr(res, REC), ptr(mask, GUARD) if n else None, None, engine.stream) == 0
    res_h, mask_h = res.cpu().numpy(), mask.cpu().numpy()
    assert (res_h[:REC] == 0xA5).all() and (res_h[2 * REC:] == 0xA5).all()
    assert (mask_h[:GUARD] == 0xA5).all() and (mask_h[GUARD + n:] == 0xA5).all()
    if n == 0:
        rec = np.frombuffer(res_h[REC:2 * REC].tobytes(), dtype=res_dtype())[0]
        assert eh.facts(rec) == dict(trials=0, best_trial=-1, status=2, n_inliers=0) and rec["n_pairs"] == 0 and np.array_equal(eh.rt(rec), eh.EYE)
    else:
        rec, m = run(x1, x2, draws, ar.THRESHOLD)
        assert res_h[REC:2 * REC].tobytes() == rec.tobytes() and np.array_equal(mask_h[GUARD:GUARD + n], m)
        assert rec["status"] == 0 and (rec["trials"] >= 100 or n == 3)


def res_dtype():
    from caelo import _ffi
    assert _ffi.ADAPTIVE_DTYPE.itemsize == REC
    return _ffi.ADAPTIVE_DTYPE


def test_same_bytes_on_every_run(run):
    x1, x2, draws, t = ar.edge_cases()["stop_129"][:4]
    first, again = run(x1, x2, draws, t), run(x1, x2, draws, t)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


TABLE = [(9, 5), (0, 1), (6, 0), (8, 5), (7, 3), (2, 2)]      # pairs that end after 5, 1, 79, 2, 0 and 1 chunks, side by side


def _edge_table_frames():
    """The eight frames of tests/test_adaptive_gpu.py and two more, made of frame 5: in frame 8 three points of ten are frame 5's,
    moved, with their descriptors, in frame 9 two of ten; the others are unrelated points.  The pair (8, 5) needs two chunks of
    trials, (9, 5) five."""
    rows8, nk8 = tg._table_frames()
    rows, nk = np.zeros((10, 1024, 64), np.float32), np.zeros(10, np.int32)
    rows[:8], nk[:8] = rows8, nk8
    rs = np.random.RandomState(78)
    for f, k, share in ((8, 180, 0.3), (9, 190, 0.2)):
        m = int(round(share * k))
        pick = rs.permutation(int(nk[5]))[:m]
        R, T = ar.random_rigid(rs)
        pts = rs.uniform(-40, 40, (k, 3)) * np.array([1.0, 1.0, 0.1])
        d = rs.uniform(-1, 1, (k, 60))
        pts[:m] = (R @ rows[5, pick, 60:63].astype(np.float64).T).T + T + 0.05 * rs.standard_normal((m, 3))
        d[:m] = rows[5, pick, 0:60] + 0.01 * rs.standard_normal((m, 60))
        order = rs.permutation(k)
        rows[f, :k, 0:60], rows[f, :k, 60:63], rows[f, :k, 63], nk[f] = d[order], pts[order], 1.0, k
    return rows, nk


def test_table_pairs_ending_after_different_numbers_of_chunks(engine, run):
    """Every record of a table whose workgroups leave the chunk loop at different times equals its single call, byte for byte."""
    rows_h, nk = _edge_table_frames()
    draws = ar.base_draws(0)
    out = engine.register_pairs_adaptive(torch.from_numpy(rows_h).to(engine.device), torch.from_numpy(nk).to(engine.device), TABLE, run.up(draws),
                                         ar.THRESHOLD)
    idx = out.pair_idx.cpu().numpy()
    for q, (a, b) in enumerate(TABLE):
        n = int(nk[a])
        assert np.array_equal(idx[q, :n], tg._argmin_f64(rows_h[a, :n, 0:60], rows_h[b, :nk[b], 0:60])), (q, a, b)
        x1, x2 = rows_h[a, :n, 60:63].astype(np.float64), rows_h[b, idx[q, :n], 60:63].astype(np.float64)
        rec, mask = run(x1, x2, draws, ar.THRESHOLD)
        assert rec.tobytes() == out.results[q].tobytes(), (q, a, b)
        assert np.array_equal(out.masks[q, :n], mask) and not out.masks[q, n:].any()
    st = {ab: (int(out.results["status"][q]), int(out.results["trials"][q])) for q, ab in enumerate(TABLE)}
    assert st[(0, 1)] == (0, 100) and st[(2, 2)] == (0, 100) and st[(6, 0)] == (1, 10000) and st[(7, 3)] == (0, 0)
    assert st[(8, 5)][0] == 0 and ar.CHUNK < st[(8, 5)][1] <= 2 * ar.CHUNK
    assert st[(9, 5)][0] == 0 and 4 * ar.CHUNK < st[(9, 5)][1] <= 5 * ar.CHUNK
